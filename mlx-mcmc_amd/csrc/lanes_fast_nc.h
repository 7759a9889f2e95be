// lanes_fast_nc.h — k_hmc_lfc: the dense launches of the fast-form HMC kernel
// k_hmc_lf (lanes_fast.h) with the chains per wave a template parameter.
//
// k_hmc_lf packs a chain pair into the halves of every f2 register.  That was
// made for the sweep; since the closed-form moments a step reads no data, and
// a dense launch of C chains is C / 2 workgroups: at C <= the device's CU
// count half of the CUs it could use hold no wave, and the packed stream costs
// a wave twice the issue of a plain one for no throughput.  k_hmc_lfc is
// k_hmc_lf's source over lf_vec<NC> instead of f2, its [0] / [1] code as loops
// over c < NC: NC = 1 compiles to plain v_*_f32 and runs a workgroup per chain.
// Only the dense 4 x 2 and 8 x 2 instantiations with NC = 1 are launched
// (run_lanes.h launch_hmc_dense); every other launch stays on k_hmc_lf, whose
// source is untouched: the one-wave kernels' schedule is sensitive to any
// change of it, and compiling them from this source cost the
// small shape 6 - 11 %.  Until they can move, the step exists twice; a change
// of the arithmetic must be made in both, and the byte equality of the two
// routes (tests/test_gpu_hmc_dense_single.py) fails when it is not.
#pragma once
#include "lanes_fast.h"

namespace mc {

// The chains of a wave, one per component: NC = 2 is f2 (the packed pair),
// NC = 1 one chain in plain v_*_f32 — the same IEEE operation per component
// either way (-ffp-contract=off: the fmas are the written ones).
template <int NC>
using lf_vec = float __attribute__((ext_vector_type(NC)));
typedef lf_vec<1> f1;
MC_DEV f1 vpin(f1 x) {
    x[0] = vpin((float)x[0]);
    return x;
}
// the chains' values a (chain 0) and b (chain 1; dropped when NC = 1)
template <int NC>
MC_DEV lf_vec<NC> lf_mk(float a, float b) {
    if constexpr (NC == 2) return (f2){a, b};
    else return (f1){a};
}
template <int NC>
MC_DEV lf_vec<NC> lf_bc(float x) {
    return lf_mk<NC>(x, x);
}
template <class V>
MC_DEV V lf_fma(V a, V b, V c) { return __builtin_elementwise_fma(a, b, c); }

// ---- one chain per wave: four values per step, one register, one float ----
// A chain's step has four wave totals to exchange: value 0 is log p (last step
// only), value 1 + k the cotangent of shared slot k (NSH = 3).  lf_rs8 carries
// them as the even pairs of eight with zeros for the partner chain; lf_rs4
// takes the four alone and leaves value v's total in row v of ONE register.
// Per value the summation tree is lf_rs8's: lane l + lane l + 32, then + lane
// l + 16, then the four DPP levels inside the row — only the register and the
// half of the wave in which a value is summed differ, and every add is of the
// same two operands (fp add is commutative), so the totals are the same bits.
// Z0: value 0 carries nothing (not a last step): v[0] is not read and row 0 of
// the result is unspecified.  (The 32-lane swap that places v[2] needs a
// partner register: a dead one, the first half of the swap before it, not a
// zero materialised per step — lf_rs8's Z01 trick.)
//
// The lane maps that go with it (checked below, at compile time):
//   lf_rs4's inputs   the 32-lane swaps pair (v[0], v[2]) and (v[1], v[3]),
//                     the 16-lane swap joins them: row r = input 2 (r & 1) +
//                     (r >> 1) of (v[0], v[2], v[1], v[3]) = value r;
//   the LDS line      per parity [slice][4] floats, value v of slice s at
//                     4 s + v, then K0[slice], K1[slice] (first / last step);
//   the publish       lane 16 v of wave s stores value v (one ds_write_b32);
//   the read          lane 16 r + c reads value r of slice c < DN (one
//                     ds_read_b32; no two lanes of the 32 readers share a bank),
//                     so after the 16-lane slice sum row r holds value r;
//   the holders       shared slot k lives in lane 16 (k + 1): its cotangent
//                     total is in its own register without a select.
// The pair kernel's holders are lanes 16, 1, 17 (lf_shlane); the own priors'
// log p must enter the log-p sum in THOSE lanes (the lane fixes the term's
// place in the tree), so the last step hands it over (k_hmc_lfc below).
constexpr int lfc_rs4_input(int v) { return v == 1 ? 2 : (v == 2 ? 1 : v); }  // value -> input
constexpr int lfc_rs4_row_input(int r) { return 2 * (r & 1) + (r >> 1); }     // row -> input
constexpr int lfc_holder(int k) { return 16 * (k + 1); }
constexpr int lfc_line_floats(int NC, int DN) { return NC == 1 ? 6 * DN : 16 * DN; }
constexpr int lfc_pub_off(int DN, int slice, int v) { return (void)DN, 4 * slice + v; }
constexpr int lfc_read_off(int DN, int lane) {
    const int row = lane >> 4, col = lane & 15;
    return 4 * (col < DN ? col : DN - 1) + row;
}
constexpr bool lfc_rs4_model(int DN, int NSH) {
    // the reduce-scatter itself, lane by lane: which input each lane holds
    int w[2][64] = {}, t[64] = {};
    for (int m = 0; m < 2; ++m)      // permlane32_swap(in[2m], in[2m+1]), halves added
        for (int l = 0; l < 64; ++l) w[m][l] = 2 * m + (l >= 32 ? 1 : 0);
    for (int l = 0; l < 64; ++l)     // permlane16_swap(w[0], w[1]), rows added
        t[l] = w[(l >> 4) & 1][32 * (l >> 5)];
    // every value lands in exactly one row, row v, which is the row model's
    for (int v = 0; v < 4; ++v) {
        int rows = 0;
        for (int r = 0; r < 4; ++r) {
            for (int c = 1; c < 16; ++c)
                if (t[16 * r + c] != t[16 * r]) return false;
            if (t[16 * r] != lfc_rs4_row_input(r)) return false;
            if (t[16 * r] == lfc_rs4_input(v)) {
                ++rows;
                if (r != v) return false;
            }
        }
        if (rows != 1) return false;
    }
    // every (slice, value) is stored by one lane of its wave, inside the value
    // floats, and read by exactly one lane of each wave
    for (int s = 0; s < DN; ++s)
        for (int v = 0; v < 4; ++v) {
            const int off = lfc_pub_off(DN, s, v);
            if (off < 0 || off >= 4 * DN) return false;
            int readers = 0;
            for (int l = 0; l < 64; ++l)
                if ((l & 15) < DN && lfc_read_off(DN, l) == off) {
                    ++readers;
                    if ((l >> 4) != v || (l & 15) != s) return false;
                }
            if (readers != 1) return false;
        }
    for (int l = 0; l < 64; ++l)     // (idle columns read in bounds)
        if (lfc_read_off(DN, l) < 0 || lfc_read_off(DN, l) >= 4 * DN) return false;
    if (4 * DN + 2 * DN != lfc_line_floats(1, DN)) return false;  // + K0[DN], K1[DN]
    // the holders: distinct lanes, each in the row of its slot's value, none
    // of them a lane where the pair route adds an own prior's log p twice
    if (NSH > 3) return false;
    for (int k = 0; k < NSH; ++k) {
        if (lfc_holder(k) < 0 || lfc_holder(k) >= 64 || (lfc_holder(k) >> 4) != 1 + k) return false;
        for (int k2 = 0; k2 < k; ++k2)
            if (lfc_holder(k2) == lfc_holder(k) || lf_shlane(k2, 0) == lf_shlane(k, 0)) return false;
    }
    return true;
}
static_assert(lfc_rs4_model(8, 3) && lfc_rs4_model(4, 3) && lfc_rs4_model(2, 3) &&
              lfc_rs4_model(16, 3), "the four-value record's lane maps");
template <bool Z0 = false>
MC_DEV float lf_rs4(const float (&v)[4]) {
    // lanes 0-31: v[1] sums, lanes 32-63: v[3] sums
    const auto r1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[1]), __float_as_uint(v[3]),
                                                     false, false);
    const float w1 = __uint_as_float(r1[0]) + __uint_as_float(r1[1]);
    // lanes 0-31: v[0] sums (Z0: unspecified), lanes 32-63: v[2] sums
    const auto r0 = __builtin_amdgcn_permlane32_swap(Z0 ? r1[0] : __float_as_uint(v[0]),
                                                     __float_as_uint(v[2]), false, false);
    const float w0 = __uint_as_float(r0[0]) + __uint_as_float(r0[1]);
    // rows 0, 2: w0's halves (v[0], v[2]); rows 1, 3: w1's (v[1], v[3])
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(w0), __float_as_uint(w1),
                                                    false, false);
    float t = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    t += lf_dpp<0xB1>(t);
    t += lf_dpp<0x4E>(t);
    t += lf_dpp<0x141>(t);
    t += lf_dpp<0x140>(t);
    return t;
}

// the lane that holds shared slot k of chain c
template <int NC>
MC_DEV constexpr int lfc_shlane(int k, int c) {
    return NC == 1 ? lfc_holder(k) : lf_shlane(k, c);
}
// every chain's value of shared slot k
template <int NC>
MC_DEV lf_vec<NC> lf_shc(float v, int k) {
    lf_vec<NC> r;
#pragma unroll
    for (int c = 0; c < NC; ++c) r[c] = rl(v, lfc_shlane<NC>(k, c));
    return r;
}

// lf_moments (lanes_fast.h) per chain of the wave
template <class V>
struct LfMomV {
    V c, R, R2, Q, n;  // (each a value broadcast to the wave's chains; R2 = 2 R)
};
template <class V>
MC_DEV void lf_moments(const LfMomV<V>& m, V th, V& M1, V& M2) {
    const V d = m.c - th;
    M1 = lf_fma(m.n, d, m.R);
    M2 = lf_fma(lf_fma(m.n, d, m.R2), d, m.Q);
}

// lf_draw_job (lanes_fast.h) for NC chains per workgroup: NC = 1 deals the NBk
// momentum blocks, then the accept draw, of the one chain — chain 0's jobs.
constexpr int lfc_draw_jobs(int D, int NC) { return NC * ((D + 3) / 4) + NC; }
constexpr LfDrawJob lfc_draw_job(int t, int D, int NC) {
    const int NBk = (D + 3) / 4;
    const bool acc = t >= NC * NBk;
    const int c = acc ? t - NC * NBk : (t >= NBk ? 1 : 0);
    return {acc, c, acc ? 0 : t - (c ? NBk : 0)};
}
// every (chain, block) and every chain's accept draw are taken exactly once
constexpr bool lfc_draw_jobs_once(int D, int lanes, int NC) {
    const int NBk = (D + 3) / 4;
    int mom[2][257] = {}, acc[2] = {};
    if (NBk > 257) return false;
    for (int tid = 0; tid < lanes; ++tid)
        for (int t = tid; t < lfc_draw_jobs(D, NC); t += lanes) {
            const LfDrawJob jb = lfc_draw_job(t, D, NC);
            if (jb.c < 0 || jb.c >= NC || jb.b < 0 || jb.b >= NBk) return false;
            if (jb.acc) ++acc[jb.c];
            else ++mom[jb.c][jb.b];
        }
    for (int c = 0; c < NC; ++c) {
        if (acc[c] != 1) return false;
        for (int b = 0; b < NBk; ++b)
            if (mom[c][b] != 1) return false;
    }
    return true;
}
static_assert(lfc_draw_jobs(1000, 2) == lf_draw_jobs(1000) && lfc_draw_jobs_once(1000, 512, 2) &&
              lfc_draw_job(300, 1000, 2).c == lf_draw_job(300, 1000).c &&
              lfc_draw_job(501, 1000, 2).acc && lf_draw_job(501, 1000).acc,
              "NC = 2: the pair kernel's job map");
static_assert(lfc_draw_jobs(1000, 1) == 251 && lfc_draw_jobs_once(1000, 512, 1) &&
              lfc_draw_jobs_once(1027, 256, 1) && lfc_draw_jobs_once(5, 256, 1) &&
              lfc_draw_jobs_once(303, 256, 1) && lfc_draw_jobs_once(1024, 512, 1),
              "one chain's jobs");

// NC — chains per wave.  2: a chain pair, one chain per half of every f2.
// 1 (dense launches only): a workgroup is one chain, blockIdx.x, in plain
// v_*_f32 — half the issue of the packed stream and none of the waits the
// compiler puts between dependent packed operations — so that a launch of at
// most as many chains as the device has CUs uses a CU per chain where the
// pairs leave half of them empty.  The chain's arithmetic and every summation
// tree are the pair kernel's for that chain; its record is the four values of
// one chain (lf_rs4 above: one register, one float per slice and value in the
// LDS line, the shared slots held in lanes 16, 32, 48), and the own priors'
// log p is added in the pair route's lanes — for an odd chain of the launch,
// chain 1 of a pair there, 32 lanes up — so the two routes' results are the
// same bytes.
template <int RS, int NSH, int NW, bool X1, int FORM, bool XL = false, int SPEC = 0, int DN = 0,
          int NC = 2>
__global__ void __launch_bounds__(64 * NW)
k_hmc_lfc(LrCtx P, RunArgs A, int64_t chain_base, int64_t n_groups, mc_chain_scalars* scal,
         float* st_q, float* st_g, float* samples, TraceDev tr, unsigned long long* xch,
         int* status, uint32_t ebase) {
    static_assert(NSH <= kLrMaxShared, "shared parameters");
    constexpr bool CF = FORM >= 0;      // the form is fixed at compile time
    static_assert(!CF || lf_nroles(FORM) == NSH, "record slots of a compile-time form");
    constexpr bool DENSE = DN > 0;
    static_assert(!DENSE || (DN == NW && DN >= 2 && DN <= kLrSlices && !X1 && !XL),
                  "dense: wave w is slice w, records through LDS");
    static_assert(DENSE && (NC == 1 || NC == 2), "k_hmc_lfc: the dense launches");
    typedef lf_vec<NC> fc;              // a value per chain of the wave
    // chains per block: wave w owns chains 2w, 2w + 1 (dense: the block's NC)
    constexpr int NB = DENSE ? NC : 2 * NW;
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
    for (int c = 0; c < 2; ++c) {  // (NC = 1: no partner — c = 1 names chain 0, never live)
        live[c] = c < NC && cbase + b0 + c < C;
        cc[c] = min(cbase + b0 + (c < NC ? c : 0), C - 1);
    }

    // LDS: (dense: the record lines [parity][slice][16] — one chain per wave:
    // [parity]{[slice][4], K0[slice], K1[slice]}, lf_rs4 above — then) the scalar
    // terms.  The slice block stays in global memory: a step reads no
    // observation (lf_moments), and the run lengths come with the constants.
    constexpr bool RS4 = NC == 1;       // the four-value record (lf_rs4)
    static_assert(!RS4 || (CF && NSH == 3 && lfc_rs4_model(DN, NSH)),
                  "one chain per wave: log p and three cotangents");
    constexpr int LW = lfc_line_floats(NC, DN);  // floats per parity
    static_assert((2 * LW) % 4 == 0, "the scalar terms' float4 copies follow the lines");
    float* const xl = smem;
    const int64_t* blk = P.blocks + 4 * (int64_t)slice;
    const float* gd = P.data + blk[0];
    const int nsweep = (int)(blk[3] & 255);
    const int ndirect = (int)((blk[3] >> 8) & 255);
    LrSterm* sst = (LrSterm*)(smem + (DENSE ? 2 * LW : 0));
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
        for (int c = 0; c < NC; ++c)
            if (k < nsl && lfc_shlane<NC>(k, c) == j) {
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
    fc q[RS], p[RS], g[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        gk[r] = P.gidx[((int64_t)slice * kLrMaxSlots + r) * 64 + j];
#pragma unroll
        for (int c = 0; c < 2; ++c) {  // (NC = 1: chain 0 again)
            R0.q[r][c] = gk[r] >= 0 ? st_q[cc[c] * D + gk[r]] : 0.0f;
            R0.g[r][c] = gk[r] >= 0 ? st_g[cc[c] * D + gk[r]] : 0.0f;
        }
        q[r] = lf_mk<NC>(R0.q[r][0], R0.q[r][1]);
        g[r] = lf_mk<NC>(R0.g[r][0], R0.g[r][1]);
        p[r] = lf_bc<NC>(0.0f);
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
    double eps[2];  // (NC = 1: [1] unused, here and below)
    fc lp;
    int nacc[2], ntot[2], wacc[2], wtot[2];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
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
    // terms, per iteration parity: z[NC][4 NBk] and the chains' accept logs.  The
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
    const int ZB = 4 * NC * NBk + 4;  // floats per parity
    static_assert(sizeof(LrSterm) % 16 == 0, "the draws' float4 stores follow the scalar terms");
    float* const zl = (float*)sst + P.n_sterms * (int)(sizeof(LrSterm) / 4);
    auto draw_block = [&](int64_t itd) {
        float* const zb = zl + (int)(itd & 1) * ZB;
        for (int t = tid; t < lfc_draw_jobs(D, NC); t += 64 * NW) {
            const LfDrawJob jb = lfc_draw_job(t, D, NC);
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
            if (acl) zb[4 * NC * NBk + c] = la;
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
    fc cnt[RS];
    LfMomV<fc> mom[RS];
    bool pdir[RS];
#pragma unroll
    for (int r = 0; r < RS; ++r) {
        float4 m = {0.f, 0.f, 0.f, 0.f};
        if (SW && r < tt[0].nslot) m = P.mom[((int64_t)slice * kLrMaxSlots + r) * 64 + j];
        len[r] = (int)m.w;
        cnt[r] = lf_bc<NC>(m.w);
        mom[r].c = vpin(lf_bc<NC>(m.x));
        mom[r].R = vpin(lf_bc<NC>(m.y));
        mom[r].R2 = vpin(lf_bc<NC>(m.y + m.y));
        mom[r].Q = vpin(lf_bc<NC>(m.z));
        mom[r].n = cnt[r];
        pdir[r] = DIR && r < tt[nsweep].nslot &&
                  ((const int32_t*)gd)[tt[nsweep].len_off + r * 64 + j] > 0;
    }
    // the terms' constants, pinned in VGPRs
    const fc sw_w = vpin(lf_bc<NC>(F.sw_w)), sw_c0 = vpin(lf_bc<NC>(F.sw_c0));
    const fc sw_cinv = vpin(lf_bc<NC>(F.sw_cinv)), sw_cinv2 = vpin(lf_bc<NC>(F.sw_cinv2)),
             sw_clogs = vpin(lf_bc<NC>(F.sw_clogs));
    const fc d_w = vpin(lf_bc<NC>(F.d_w)), d_c0 = vpin(lf_bc<NC>(F.d_c0)), d_m = vpin(lf_bc<NC>(F.d_m));
    // (one slot: the direct term's weight per lane, zero where the lane's
    // parameter has no direct term)
    const fc d_w1 = vpin(lf_bc<NC>(pdir[0] ? F.d_w : 0.0f));
    const fc d_cinv = vpin(lf_bc<NC>(F.d_cinv)), d_cinv2 = vpin(lf_bc<NC>(F.d_cinv2)),
             d_clogs = vpin(lf_bc<NC>(F.d_clogs));
    const fc half = lf_bc<NC>(0.5f), one = lf_bc<NC>(1.0f);
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
    auto lput = [&](int par, int off, float v) { xl[par * LW + off] = v; };
    // one chain per wave (lf_rs4): lane 16 v stores value v of this wave's
    // slice; lane 1 / lane 17 the K0 / K1 float of a first / last step; lane
    // 16 r + c reads value r of slice c, rows 0 / 1 the K0 / K1 floats
    const int pub4_off = lfc_pub_off(DN, slice, row);
    const bool pub4 = col == 0, pub4_mid = col == 0 && row > 0;
    const int lrd4 = lfc_read_off(DN > 0 ? DN : 1, j);
    const int lrdk = 4 * DN + (row & 1) * DN + min(col, S - 1);
    // publishing: lanes 16 r + n (n < NRS * 2) hold pair 8 (n / 2) + 4 (n % 2) + perm[r]
    const int pub_pair = (col < 2 * NRS) ? 8 * (col >> 1) + 4 * (col & 1) + lf_row(row) : -1;
    // (NC = 1: the odd pairs, chain 1's, are neither published nor polled)
    const bool pub_rec = pub_pair >= 0 && pub_pair < NV && (NC == 2 || !(pub_pair & 1));
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
        if (X1 || !poll_lane || pr >= NPAIR || (NC == 1 && (pr & 1))) continue;
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
    fc nx_z[RS];
    float nx_sh = 0.0f, nx_lu[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < RS; ++r) nx_z[r] = lf_bc<NC>(0.0f);
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
            nx_z[r] = lf_mk<NC>(fetch(word & 63, comp), fetch((word >> 6) & 63, comp));
        }
        nx_sh = fetch(sh_src, xg & 3);
    };
    if (DRAW_AHEAD && rngp && cfg.iter_count > 0) draw_plan(cfg.iter_begin);
    for (int64_t it = cfg.iter_begin; it < it_end && ok; ++it) {
        MC_STAMP_DECL
        const bool warm = it < cfg.num_warmup;
        float hs[2], es[2];  // (NC = 1: [1] is [0], read by no lane)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (it == cfg.num_warmup) {  // hmc.py:175-180
                wacc[c] = nacc[c];
                wtot[c] = ntot[c];
                nacc[c] = 0;
                ntot[c] = 0;
            }
            hs[c] = (float)(0.5 * eps[c]);
            es[c] = (float)eps[c];
        }
        if constexpr (NC == 1) {
            hs[1] = hs[0];
            es[1] = es[0];
        }
        const fc h = vpin(lf_mk<NC>(hs[0], hs[1])), e = vpin(lf_mk<NC>(es[0], es[1]));
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
        fc k0p = lf_bc<NC>(0.0f);
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
                // (the plan is made for a pair: with NC = 1 the lanes of chain
                // 1's jobs, csel = 1, draw for chain 0 again and nobody fetches
                // from them — wasted work once per iteration, same bits)
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
                    const fc zz = lf_mk<NC>(fetch(word & 63, comp), fetch((word >> 6) & 63, comp));
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
#pragma unroll
            for (int c = 0; c < NC; ++c) logu_acc[c] = zb[4 * NC * NBk + c];
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int gi = max(gk[r], 0);
                fc z;
#pragma unroll
                for (int c = 0; c < NC; ++c) z[c] = zb[4 * NBk * c + gi];
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
                fc z;
#pragma unroll
                for (int c = 0; c < NC; ++c) z[c] = normal_of(gk[r], cc[c]);
                p[r] = z;
                if (lead) k0p += z * z;
            }
            sh.p = xon ? normal_of(xg, xch_id) : 0.0f;
        }
        const float K0w[2] = {wave_sum(k0p[0]), wave_sum(k0p[NC - 1])};
        float k0s[2] = {0.f, 0.f};  // the shared parameters' part, in slot order
        {
            const float p2 = sh.p * sh.p;
            for (int k = 0; k < nsl; ++k) {
#pragma unroll
                for (int c = 0; c < NC; ++c) k0s[c] += rl(p2, lfc_shlane<NC>(k, c));
            }
        }
        fc q0[RS], g0[RS];
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            q0[r] = q[r];
            g0[r] = g[r];
        }
        const float q0s = sh.q, g0s = sh.g;
        fc lpn = lp;
        float K0[2] = {0.f, 0.f}, K1[2] = {0.f, 0.f};
        MC_STAMP(5);
        // (the two half kicks of consecutive steps stay separate roundings, as
        // the reference's; their common product h * g is formed once)
        auto drift_private = [&](bool second_half) {
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const fc hg = h * g[r];
                fc pj = p[r];
                if (second_half) pj = pj + hg;  // end of the previous step
                pj = pj + hg;
                p[r] = pj;
                q[r] = q[r] + e * pj;
            }
        };
        // The own prior's gradient at sh.v.  A pair: formed with sh.v, below.
        // One chain per wave: formed by the step that adds it, behind its LDS
        // read — off the chain reciprocal -> broadcast -> next finish that
        // drift_shared heads (profiles/lf_rs4; the same expression on the
        // same operand either way).
        float gown = 0.0f;
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
            if constexpr (!RS4) gown = vpin(own_grad(sh.v));  // for the step at this position
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
            const fc z0 = lf_bc<NC>(0.0f);
            fc lpp = z0, cs = z0, cm = z0, cd = z0;
            bool lpp0 = true, cs0 = true, cm0 = true, cd0 = true;
            bool g0r[RS];
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                g[r] = lf_bc<NC>(0.0f);
                g0r[r] = true;
            }
            auto acc = [](fc& s, bool& first, fc v) {
                s = first ? v : s + v;
                first = false;
            };
            // (a shared scale's 1/s^2 is squared here from its 1/s: the
            // holding lane's sh.iv = sh.is * sh.is, the same rounding)
            fc M2[RS];
            if (SW) {
                const fc is = SWS ? lf_shc<NC>(sh.is, ksw) : sw_cinv;
                const fc iv = SWS ? is * is : sw_cinv2;
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    const bool on = len[r] != 0;
                    const fc z = lf_bc<NC>(0.0f);
                    // both moment sums at q[r] from the run's constants (the
                    // drift to the next position follows this finish); an
                    // empty lane's are zeros whatever its position is
                    fc m1, m2;
                    lf_moments(mom[r], q[r], m1, m2);
                    const fc M1r = on ? m1 : z;
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
                        const fc lg = SWS ? lf_shc<NC>(sh.lg, ksw) : sw_clogs;
                        const fc lpt = cnt[r] * (sw_c0 - lg) - (half * M2[r]) * iv;
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
                const fc um = DM ? lf_shc<NC>(sh.v, kdm) : d_m;
                const fc is = DS ? lf_shc<NC>(sh.is, kds) : d_cinv;
                const fc iv = DS ? is * is : d_cinv2;
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    // one slot: a lane without the term weighs it by zero (its
                    // cotangent items 0 * finite, its gradient g - 0) instead
                    // of branching around it under an exec mask
                    if (RS > 1 && !pdir[r]) continue;
                    const fc dw = RS == 1 ? d_w1 : d_w;
                    const fc d = q[r] - um;
                    const fc s2 = d * d;
                    const fc u = dw * (d * iv);
                    acc(g[r], g0r[r], -u);
                    acc(cm, cm0, u);
                    acc(cd, cd0, dw * ((s2 * iv - one) * is));
                    if (lst) {
                        const fc lg = DS ? lf_shc<NC>(sh.lg, kds) : d_clogs;
                        const fc lpt = one * (d_c0 - lg) - (half * s2) * iv;
                        acc(lpp, lpp0, dw * lpt);
                    }
                }
            }
            // a replicated parameter's gradient: the sum of its lanes' partials
            static_assert(NC == 2 || (SPEC & LFS_REP1) != 0, "one chain per wave: rep == 1");
            // (the identity terms below are not handed up for odd chains as the
            // own priors are: one chain per wave has no transformed parameter)
            static_assert(NC == 2 || (SPEC & LFS_NOXF) != 0, "one chain per wave: no transform");
            if constexpr (NC == 2) {
                if (rep > 1) {
#pragma unroll
                    for (int r = 0; r < RS; ++r) {
                        float a = g[r][0], b = g[r][1];
                        grp_sum2(a, b, rep);
                        g[r] = (fc){a, b};
                    }
                }
            }
            // the own prior of this lane's shared parameter (moment form with
            // the constant scale's reciprocals, as the sliced terms); its log p
            // enters slice 0's record
            float g_own = gown;  // (a pair: formed in drift_shared; one chain: below)
            {
                if (lst) {
                    const float v = sh.v;
                    const float d = v - o_m;
                    const bool out = own.hn && !(v >= 0.0f);
                    const float d2 = d * d;
                    const float lpe = out ? -__builtin_inff() : o_c0l - (0.5f * d2) * o_cinv2;
                    const float lp_own = o_wn * lpe;
                    if constexpr (NC == 2) {
                        if (own_lp0) lpp[0] += lp_own;
                        if (own_lp1) lpp[1] += lp_own;
                    } else {
                        // On the pair route the own priors enter the log-p sum
                        // in the holders' lanes lf_shlane(k, 0) (16, 1, 17) —
                        // for an odd chain of the launch, chain 1 of its pair
                        // there, in lf_shlane(k, 1), 32 above — and the lane
                        // fixes a term's place in the summation tree.
                        static_assert(lf_shlane(0, 1) == lf_shlane(0, 0) + 32 &&
                                      lf_shlane(1, 1) == lf_shlane(1, 0) + 32 &&
                                      lf_shlane(2, 1) == lf_shlane(2, 0) + 32 &&
                                      lf_shlane(3, 1) == lf_shlane(3, 0) + 32, "chain 1's holders");
                        // This route's holders are the lanes lfc_holder(k) (the
                        // rows of lf_rs4's totals): each hands its term to the
                        // pair route's lane of its slot and chain, so the wave
                        // total is summed in the pair route's order.
                        const bool odd = (cbase & 1) != 0;
                        const float lpo = own_lp0 ? lp_own : 0.0f;
#pragma unroll
                        for (int k = 0; k < NSH; ++k) {
                            const float lpk = rl(lpo, lfc_holder(k));
                            const bool onk =
                                __builtin_amdgcn_readlane(own_lp0 ? 1 : 0, lfc_holder(k)) != 0;
                            if (onk && j == lf_shlane(k, 0) + (odd ? 32 : 0)) lpp[0] += lpk;
                        }
                    }
                    // the identity terms over the raw parameter (log-Jacobians)
                    if (hxf && slice == 0 && xon) {
                        if (xc == 0) lpp[0] += xid * sh.q;
                        else if constexpr (NC == 2) lpp[1] += xid * sh.q;
                    }
                }
            }
            MC_STAMP(1);
            // wave totals, reduce-scattered: pair P = 2 slot + chain
            float xr[2 * NRS];
            float xr4 = 0.0f;  // one chain per wave: value v's total in row v
            if constexpr (RS4) {
                float v[4];
                v[0] = lpp[0];
                v[1 + lf_slot_sws(FORM)] = (FORM & LF_SWS) ? cs[0] : 0.0f;
                v[1 + lf_slot_dm(FORM)] = (FORM & LF_DM) ? cm[0] : 0.0f;
                v[1 + lf_slot_ds(FORM)] = (FORM & LF_DS) ? cd[0] : 0.0f;
                xr4 = lst ? lf_rs4(v) : lf_rs4<true>(v);  // (no log p but on the last step)
#pragma unroll
                for (int x = 0; x < 2 * NRS; ++x) xr[x] = 0.0f;
            } else {
                float v[8 * NRS];
#pragma unroll
                for (int x = 0; x < 8 * NRS; ++x) v[x] = 0.0f;
                // (NC = 1: the odd pairs stay the zeros above)
#pragma unroll
                for (int c = 0; c < NC; ++c) v[c] = lpp[c];
                if constexpr (CF) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        if (FORM & LF_SWS) v[2 + 2 * lf_slot_sws(FORM) + c] = cs[c];
                        if (FORM & LF_DM) v[2 + 2 * lf_slot_dm(FORM) + c] = cm[c];
                        if (FORM & LF_DS) v[2 + 2 * lf_slot_ds(FORM) + c] = cd[c];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < NSH; ++k)
#pragma unroll
                        for (int c = 0; c < NC; ++c)
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
                fc k1p = lf_bc<NC>(0.0f);
#pragma unroll
                for (int r = 0; r < RS; ++r) {
                    const fc pj = p[r] + h * g[r];
                    if (lead) k1p += pj * pj;
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) k1w[c] = wave_sum(k1p[c]);
            }
            ++epoch;
            const int par = PAR >= 0 ? PAR : (int)(epoch & 1);
            if constexpr (RS4 && !FIRST && !LAST) {
                // an intermediate step: the three cotangents, from the one
                // register, at addresses fixed per launch and parity
                if (pub4_mid) lput(par, pub4_off, xr4);
            } else if constexpr (RS4) {
                // one store instruction: the values (log p on the last step
                // only) and the K float of a first / last step
                int po = (pub4 && (lst || row > 0)) ? pub4_off : -1;
                float pv = xr4;
                if (col == 1) {
                    if (FIRST && row == 0) {
                        po = 4 * DN + slice;
                        pv = K0w[0];
                    }
                    if (LAST && row == 1) {
                        po = 5 * DN + slice;
                        pv = k1w[0];
                    }
                }
                if (po >= 0) lput(par, po, pv);
            } else if constexpr (!X1 && !FIRST && !LAST) {
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
                if (col == 2 * NRS || (NC == 2 && col == 2 * NRS + 1)) {
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
                if constexpr (RS4) {
                    // one float per lane (a first / last step: and its K float)
                    const float va = xl[par * LW + lrd4];
                    const float vk = kstep ? xl[par * LW + lrdk] : 0.0f;
                    // while the reads are on their way: the own prior's
                    // gradient at this step's shared value
                    g_own = own_grad(vpin(sh.v));
                    // (idle columns enter the 16-lane slice sums as zeros)
                    vals[0] = poll_lane ? va : 0.0f;
                    const bool ndk = poll_lane && ((FIRST && row == 0) || (LAST && row == 1));
                    if constexpr (NPASS > 1) vals[1] = ndk ? vk : 0.0f;
                } else {
#pragma unroll
                    for (int ps = 0; ps < NPASS; ++ps) {
                        const bool nd = ((need >> ps) & 1u) != 0u;
                        const float v =
                            (ps < NPASS_V || kstep) ? xl[par * LW + lpoll + 4 * ps] : 0.0f;
                        vals[ps] = nd ? v : 0.0f;
                    }
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
            } else if constexpr (RS4) {
                // value r in row r of tot[0]; K0 / K1 in rows 0 / 1 of tot[1]
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps) {
                    float t = ps < 2 ? vals[ps] : 0.0f;
                    if (ps == 0 || (ps == 1 && kstep)) {
                        t += lf_dpp<0xB1>(t);
                        t += lf_dpp<0x4E>(t);
                        t += lf_dpp<0x141>(t);
                        t += lf_dpp<0x140>(t);
                    }
                    tot[ps] = t;
                }
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
#pragma unroll
                for (int c = 0; c < NC; ++c) lpn[c] = rl(tot[0], 16 * lf_row(c)) + lp_const;
            }
            {
                float gx = 0.0f;
                if constexpr (RS4) {
                    gx = tot[0];  // lane 16 (k + 1) holds slot k: its own row's total
                } else {
#pragma unroll
                    for (int ps = 0; ps < NPASS_V; ++ps)
                        if (col == ps) gx = tot[ps];  // lane 16 row + P / 4 holds pair P
                }
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
                } else if constexpr (RS4) {
                    K0[0] = rl(tot[1], 0);
                } else {
                    K0[0] = rl(tot[p0 / 4], 16 * lf_row(p0));
                    if constexpr (NC == 2) K0[1] = rl(tot[p1 / 4], 16 * lf_row(p1));
                }
            }
            if constexpr (LAST) {
                constexpr int p0 = NV + 2, p1 = NV + 3;
                if constexpr (X1) {
                    K1[0] = k1w[0];
                    K1[1] = k1w[1];
                } else if constexpr (RS4) {
                    K1[0] = rl(tot[1], 16);
                } else {
                    K1[0] = rl(tot[p0 / 4], 16 * lf_row(p0));
                    if constexpr (NC == 2) K1[1] = rl(tot[p1 / 4], 16 * lf_row(p1));
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
#pragma unroll
                for (int c = 0; c < NC; ++c) k1s[c] += rl(p2, lfc_shlane<NC>(k, c));
            }
        }
        bool acc[2];
        if constexpr (NC == 1) acc[1] = false;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
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
            q[r] = lf_mk<NC>(acc[0] ? q[r][0] : q0[r][0],
                             acc[NC - 1] ? q[r][NC - 1] : q0[r][NC - 1]);
            g[r] = lf_mk<NC>(acc[0] ? g[r][0] : g0[r][0],
                             acc[NC - 1] ? g[r][NC - 1] : g0[r][NC - 1]);
        }
        if (!(xc ? acc[1] : acc[0])) {
            sh.q = q0s;
            sh.g = g0s;
        }
        if (!warm && samples != nullptr) {
            const int64_t s = it - cfg.num_warmup - cfg.sample_begin;
            if (s >= 0 && s < cfg.sample_capacity) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
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
    for (int c = 0; c < NC; ++c) {
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
