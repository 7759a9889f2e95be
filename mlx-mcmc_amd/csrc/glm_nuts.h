// glm_nuts.h — NUTS for design-matrix GLMs on the MFMA gradient kernel of glm.h.
//
// A tick is one k_glm_grad launch at every chain's pending position and one
// k_glm_nuts_step launch, which moves every chain of a block by one leaf of its
// own tree.  The step kernel restates nuts.h's iterative post-order walk
// (nuts.py:137-319; the same f32 operations per element, Philox addressing and
// NaN rules) with the walk's loop state kept in memory between launches instead
// of in a persistent kernel's registers:
//   1  finish the pending leaf: log p and the gradient from the S partial blocks
//      plus the priors, second half kick, H', n', s', alpha; the leaf becomes
//      the trajectory end in the tree's direction
//   2  subtree bookkeeping: first-leaf slot min(tz(k), depth), candidate pool,
//      and for every level whose bit of k + 1 closes a second half the merge
//      uniform, the candidate choice and the U-turn test over the merged subtree
//   3  a complete (or failed) subtree: top-level accept into the chain state,
//      n += n', the U-turn test over the trajectory ends, then the next depth
//      with a new direction or the end of the iteration
//   4  iteration end: sample row, dual averaging, counters, trace; if the window
//      has more iterations the next one's momentum, H0, slice and direction
//   5  the next leaf's first half kick and drift, into the pending momentum and
//      the chain's column of qT
// Chains advance asynchronously: each carries its own iteration number and tree
// state, so in one tick a chain may build leaf 5 of a depth-3 subtree of
// iteration 17 while its neighbour in the MFMA column block starts iteration
// 19.  A chain is one MFMA column and columns never mix, so the gradient kernel
// does not care; a window costs the largest per-chain total of leaves.  A chain
// that has finished the window's last iteration is done: it leaves its column of
// qT alone and its gradient is computed and ignored.
//
// Layout (k_glm_hmc_step's): one workgroup per block of 32 chains, thread (j =
// tid % 32: the chain, pr = tid / 32: the stripe) owns the elements GLM_FOR_OWNED
// gives it in EVERY vector, so no vector element ever crosses threads; the 8
// threads of a chain compute the chain's scalar decisions redundantly from the
// same reduced values and stripe 0 stores them.  The arena is chain-minor,
// [chain block][vector][D][32]: nuts.h's nuts_arena_vectors(MAXJ) vectors (ends,
// first leaves, candidate pool) plus the pending half-kicked momentum.  The walk
// state is kGlmNutsWords words per chain, chain-minor as well.  Between launch
// windows only mc_chain_scalars, st_q and st_g carry state.
//
// Control flow is barrier-uniform: a chain's data-dependent branch (done,
// subtree failed, no merge at this level) masks its work and never skips a
// barrier; the merge loop runs to the workgroup's maximum of the levels any of
// its chains closes (through LDS), and both U-turn dots of a level go through
// one reduction round for all 32 chains.
#pragma once
#include "glm.h"
#include "nuts.h"

namespace mc {

enum { GLM_NUTS_START = 0, GLM_NUTS_TICK = 1 };

// the walk state of a chain: word w of chain j of a block at [w * 32 + j]
enum {
    NW_IO = 0,  // iteration, counted from the window's iter_begin
    NW_DEPTH,   // j of nuts.h: the depth of the subtree being built
    NW_K,       // its pending leaf
    NW_DIR,
    NW_N,
    NW_CAND,
    NW_CN,
    NW_FREE,  // free slots of the candidate pool
    NW_NALPHA,
    NW_LEAVES,
    NW_DIV,
    NW_H0,
    NW_LOGU,      // double: two words
    NW_ASUM = NW_LOGU + 2,  // double
    NW_DONE = NW_ASUM + 2,
    NW_PEND,  // per level: the parked first half's (pool slot << 24) | n'
    NW_POOL_LP = NW_PEND + kMaxTreeDepth,
    kGlmNutsWords = NW_POOL_LP + kMaxTreeDepth + 2
};

// the sums of a and b over the 8 threads of a chain, in stripe order, in one round
MC_DEV void glm_chain_sum2(float a, float b, float (*red)[kGlmStripes][kGlmChains], int pr, int j,
                           float& sa, float& sb) {
    red[0][pr][j] = a;
    red[1][pr][j] = b;
    __syncthreads();
    sa = 0.0f;
    sb = 0.0f;
#pragma unroll
    for (int k = 0; k < kGlmStripes; ++k) {
        sa += red[0][k][j];
        sb += red[1][k][j];
    }
    __syncthreads();
}

// the slice variable log u of nuts.h (nuts.py:234-237) from H0 and the f32 log U
MC_DEV double glm_nuts_slice(float H0, float log_uni, int slice_mode) {
    const double log_u = (double)(-H0) + (double)log_uni;
    if (slice_mode != 0) return log_u;
    const float x = (float)log_u;
    const double ed = exp((double)x);
    float uf;
    if (ed < 1.1754943508222875e-38)  // f32 gradual underflow, round-half-even
        uf = (float)(rint(ed * 7.1362384635297994e+44) * 1.4012984643248171e-45);
    else
        uf = (float)ed;
    return (uf == 0.0f) ? -__builtin_inf() : (double)mc_logf_ref(uf);
}

MC_DEV double glm_nuts_ld(const uint32_t* sw, int w) {
    const uint64_t u = (uint64_t)sw[w * 32] | ((uint64_t)sw[(w + 1) * 32] << 32);
    return __longlong_as_double((long long)u);
}
MC_DEV void glm_nuts_st(uint32_t* sw, int w, double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    sw[w * 32] = (uint32_t)u;
    sw[(w + 1) * 32] = (uint32_t)(u >> 32);
}

// phase GLM_NUTS_START: before a window's first gradient launch, every chain's
// first iteration (step 4's new-iteration part) and first leaf (step 5) from the
// state's own gradient; with max_tree_depth = 0 the whole window (no iteration
// has a leaf).  phase GLM_NUTS_TICK: steps 1-5 after a gradient launch at qT.
// cnt[chain block]: the block's chains that are not done after this launch.
template <int = 0>
__global__ void __launch_bounds__(256)
k_glm_nuts_step(GlmDev G, RunArgs A, int phase, mc_chain_scalars* scal, float* st_q, float* st_g,
                float* samples, TraceDev tr, float* qT, float* arena, uint32_t* sblk, int32_t* cnt,
                GlmPart R0) {
    __shared__ float red[2][kGlmStripes][kGlmChains];
    __shared__ int lv[kGlmChains];
    const mc_run_config& cfg = A.cfg;
    const int cb = blockIdx.x, j = threadIdx.x & 31, pr = threadIdx.x >> 5;
    const int64_t c = (int64_t)cb * kGlmChains + j;
    const bool live = c < cfg.num_chains;
    const int D = G.D;
    const int MAXJ = cfg.max_tree_depth;
    const int NV = (int)nuts_arena_vectors(MAXJ) + 1;
    const int VF = 6, VP = 6 + 2 * (MAXJ + 1), VR = NV - 1;  // first leaves, pool, pending r
    float* qt = qT + (int64_t)cb * D * 32 + j;  // element d at qt[d * 32]
    float* ar = arena + (int64_t)cb * NV * D * 32 + j;
    auto V = [&](int v, int d) -> float& { return ar[((int64_t)v * D + d) * 32]; };
    uint32_t* sw = sblk + (int64_t)cb * kGlmNutsWords * 32 + j;
    float* sq = st_q + c * D;
    float* sg = st_g + c * D;
    GlmPart R = R0;
    R.part += (int64_t)cb * ((G.Pp + kGlmExtra) * 32);
    const uint32_t chain_id = (uint32_t)(cfg.chain_offset + c);

    mc_chain_scalars sc = {};
    if (live) sc = scal[c];
    int io = 0, depth = 0, k = 0, dir = 1, n = 1, cand = 0, cn = 0, nalpha = 0, leaves = 0, ndiv = 0;
    uint32_t freem = 0;
    float H0 = 0.0f;
    double logu = 0.0, asum = 0.0;
    bool done = !live;
    if (phase == GLM_NUTS_TICK && live) {
        io = (int)sw[NW_IO * 32];
        depth = (int)sw[NW_DEPTH * 32];
        k = (int)sw[NW_K * 32];
        dir = (int)sw[NW_DIR * 32];
        n = (int)sw[NW_N * 32];
        cand = (int)sw[NW_CAND * 32];
        cn = (int)sw[NW_CN * 32];
        freem = sw[NW_FREE * 32];
        nalpha = (int)sw[NW_NALPHA * 32];
        leaves = (int)sw[NW_LEAVES * 32];
        ndiv = (int)sw[NW_DIV * 32];
        H0 = __uint_as_float(sw[NW_H0 * 32]);
        logu = glm_nuts_ld(sw, NW_LOGU);
        asum = glm_nuts_ld(sw, NW_ASUM);
        done = sw[NW_DONE * 32] != 0;
    }
    // what the chain does in the rest of this launch
    bool f_itend = false, f_newit = phase == GLM_NUTS_START && live, f_newdepth = false,
         f_leaf = false;

    if (phase == GLM_NUTS_TICK) {
        const bool act = !done;
        const uint32_t it = (uint32_t)(cfg.iter_begin + io);
        const float h = (float)(0.5 * ((double)dir * sc.step_size));
        const int E = dir > 0 ? 3 : 0;  // the end in the tree's direction: q, r, g at E, E + 1, E + 2
        // ---- 1. the pending leaf; it is parked as a candidate and, if it opens a
        // subtree of level >= 1, as that subtree's first leaf
        const int f = freem ? __builtin_ctz(freem) : 0;
        const bool opens = depth >= 1 && (k & 1) == 0;
        const int fslot = k == 0 ? depth : __builtin_ctz((uint32_t)k);
        float kl = 0.0f, lpp = 0.0f;
        if (act) {
            GLM_FOR_OWNED(D) {
                const float qd = qt[d * 32];
                float g = glm_like_grad(G, R, j, d, qd);
                glm_prior(G, d, qd, g, lpp);
                const float pj = V(VR, d) + h * g;  // second half kick
                kl += pj * pj;
                V(E, d) = qd;
                V(E + 1, d) = pj;
                V(E + 2, d) = g;
                V(VP + 2 * f, d) = qd;
                V(VP + 2 * f + 1, d) = g;
                if (opens) {
                    V(VF + 2 * fslot, d) = qd;
                    V(VF + 2 * fslot + 1, d) = pj;
                }
            }
        }
        const float ks = glm_chain_sum(kl, red[0], pr, j);
        const float lps = glm_chain_sum(lpp, red[0], pr, j);
        bool s_sub = true;
        int nl = 0;  // levels whose second half this leaf closes
        float lpl = 0.0f;
        if (act) {
            lpl = (G.lp_const + glm_part_sum(R, G.Pp + 2, j)) + lps;
            const float Hl = -lpl + 0.5f * ks;
            ++leaves;
            const int n_leaf = (logu <= (double)(-Hl)) ? 1 : 0;
            const bool s_leaf = logu < (double)(1000.0f - Hl);
            const double a = (double)mc_expf_ref(-Hl + H0);
            asum += (a < 1.0) ? a : 1.0;
            nalpha += 1;
            if (!s_leaf) ndiv += 1;
            freem &= ~(1u << f);
            if (pr == 0) sw[(NW_POOL_LP + f) * 32] = __float_as_uint(lpl);
            s_sub = s_leaf;
            if (s_leaf) {
                cand = f;
                cn = n_leaf;
                nl = min((int)__builtin_ctz((uint32_t)(k + 1)), depth);
            }
        }
        // ---- 2. merge completed subtrees upward, to the workgroup's deepest merge
        if (pr == 0) lv[j] = nl;
        __syncthreads();
        int L = 0;
        for (int i = 0; i < kGlmChains; ++i) L = max(L, lv[i]);
        __syncthreads();
        for (int l = 0; l < L; ++l) {
            const bool cl = act && s_sub && l < nl;
            float a = 0.0f, b = 0.0f;
            if (cl) {
                const uint32_t pw = sw[(NW_PEND + l) * 32];
                const int pidx = (int)(pw >> 24), pn = (int)(pw & 0xffffffu);
                const mc_u32x4 rm = mc_draw(cfg.seed, chain_id, it, MC_RNG_TAG_MERGE,
                                            (uint32_t)depth, ((uint32_t)l << 20) | (uint32_t)k);
                const double den = (double)(pn + cn) > 1.0 ? (double)(pn + cn) : 1.0;
                // U < cn / den (nuts.py:205) as U * den < cn: exact in f64 (nuts.h)
                if ((double)mc_u01_f32(rm.x) * den < (double)cn) {
                    freem |= 1u << pidx;
                } else {
                    freem |= 1u << cand;
                    cand = pidx;
                }
                cn = pn + cn;
                // U-turn over the merged level-(l + 1) subtree: its first leaf and the end
                const int k0 = k + 1 - (2 << l);
                const int slot = k0 == 0 ? depth : __builtin_ctz((uint32_t)k0);
                GLM_FOR_OWNED(D) {
                    const float bq = V(VF + 2 * slot, d), br = V(VF + 2 * slot + 1, d);
                    const float eq = V(E, d), er = V(E + 1, d);
                    const float dd = dir > 0 ? eq - bq : bq - eq;  // q+ - q-
                    a += dd * (dir > 0 ? br : er);                 // . r-
                    b += dd * (dir > 0 ? er : br);                 // . r+
                }
            }
            float dm, dp;
            glm_chain_sum2(a, b, red, pr, j, dm, dp);
            if (cl && !(dm >= 0.0f && dp >= 0.0f)) s_sub = false;
        }
        bool complete = false;
        if (act) {
            if (s_sub && nl < depth && pr == 0)  // a first half: parked at its level
                sw[(NW_PEND + nl) * 32] = ((uint32_t)cand << 24) | (uint32_t)cn;
            complete = !s_sub || nl == depth;  // (any s = false ends the subtree at once)
        }
        // ---- 3. top level (nuts.py:262-284)
        float a = 0.0f, b = 0.0f;
        if (act && complete) {
            const mc_u32x4 rd = mc_draw(cfg.seed, chain_id, it, MC_RNG_TAG_DEPTH, (uint32_t)depth, 0);
            const double den = (double)n > 1.0 ? (double)n : 1.0;
            if (s_sub && (double)mc_u01_f32(rd.y) * den < (double)cn) {
                GLM_FOR_OWNED(D) {
                    sq[d] = V(VP + 2 * cand, d);
                    sg[d] = V(VP + 2 * cand + 1, d);
                }
                // (this leaf's log p is stored by stripe 0 in this launch: not read back)
                sc.logp = cand == f ? lpl : __uint_as_float(sw[(NW_POOL_LP + cand) * 32]);
            }
            n += cn;
            GLM_FOR_OWNED(D) {
                const float dd = V(3, d) - V(0, d);
                a += dd * V(1, d);
                b += dd * V(4, d);
            }
        }
        float dm, dp;
        glm_chain_sum2(a, b, red, pr, j, dm, dp);
        if (act && complete) {
            const bool s = s_sub && dm >= 0.0f && dp >= 0.0f;
            depth += 1;
            if (s && depth < MAXJ) f_newdepth = true;
            else f_itend = true;
        } else if (act) {
            k += 1;
            f_leaf = true;
        }
    }

    // ---- 4. iteration end and the next iteration's start.  One turn, except with
    // max_tree_depth = 0, where START runs the window's iterations: start, end,
    // start, ... (a uniform trip count)
    const int turns = (phase == GLM_NUTS_START && MAXJ == 0) ? (int)cfg.iter_count + 1 : 1;
    for (int turn = 0; turn < turns; ++turn) {
        if (f_itend) {
            const int64_t it = cfg.iter_begin + io;
            const bool warm = it < cfg.num_warmup;
            const double eps_used = sc.step_size;
            const double alpha = asum / (nalpha > 1 ? (double)nalpha : 1.0);
            sc.n_grad += leaves;
            sc.n_divergent += ndiv;
            sc.alpha_sum += alpha;
            sc.n_accept += (alpha > 0.5) ? 1 : 0;
            sc.n_total += 1;
            sc.depth_sum += depth;
            if (warm && cfg.adapt_step_size) {  // dual averaging, nuts.py:299-310
                const double m = (double)it;
                const double eta = 1.0 / (m + 10.0);
                sc.h_bar = (1.0 - eta) * sc.h_bar + eta * (cfg.target_accept - alpha);
                const float lf = sc.mu - (float)(sqrt(m + 1.0) / 0.05 * sc.h_bar);
                double le = (double)lf;
                if (10.0 < le) le = 10.0;
                if (-10.0 > le) le = -10.0;
                const double eps = (double)mc_expf_ref((float)le);
                const double m_eta = pow(m + 1.0, -0.75);
                const double lb = m_eta * log(eps) + (1.0 - m_eta) * log(sc.step_size_bar);
                sc.step_size_bar = (double)mc_expf_ref((float)lb);
                sc.step_size = eps;
            }
            if (!warm && samples != nullptr) {
                const int64_t si = it - cfg.num_warmup - cfg.sample_begin;
                if (si >= 0 && si < cfg.sample_capacity) {
                    float* out = samples + (c * cfg.sample_capacity + si) * (int64_t)D;
                    GLM_FOR_OWNED(D) out[d] = sq[d];  // (written by this thread)
                }
            }
            const int64_t ti = it - tr.iter_begin;
            if (pr == 0 && ti >= 0 && ti < tr.capacity) {
                const int64_t o = c * tr.capacity + ti;
                if (tr.accepted) tr.accepted[o] = (alpha > 0.5) ? 1 : 0;
                if (tr.accept_stat) tr.accept_stat[o] = (float)alpha;
                if (tr.step_size) tr.step_size[o] = eps_used;
                if (tr.energy) tr.energy[o] = H0;
                if (tr.tree_depth) tr.tree_depth[o] = depth;
                if (tr.n_leapfrog) tr.n_leapfrog[o] = leaves;
            }
            io += 1;
            f_itend = false;
            if (io >= cfg.iter_count) done = true;
            else f_newit = true;
        }
        const uint32_t it = (uint32_t)(cfg.iter_begin + io);
        float kp = 0.0f;
        if (f_newit) {
            if ((int64_t)it == cfg.num_warmup) {  // nuts.py:318-319, 328-330
                if (cfg.adapt_step_size) sc.step_size = sc.step_size_bar;
                sc.warmup_accept = sc.n_accept;
                sc.warmup_total = sc.n_total;
                sc.warmup_depth_sum = sc.depth_sum;
                sc.n_accept = 0;
                sc.n_total = 0;
                sc.depth_sum = 0;
            }
            // momentum into both ends, kinetic energy (nuts.py:223-231)
            for (int m = pr; 4 * m < D; m += kGlmStripes) {
                const mc_u32x4 r = mc_draw(cfg.seed, chain_id, it, MC_RNG_TAG_MOMENTUM, 0,
                                           (uint32_t)m);
                float z[4];
                mc_box_muller(r.x, r.y, &z[0], &z[1]);
                mc_box_muller(r.z, r.w, &z[2], &z[3]);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int d = 4 * m + kk;
                    if (d < D) {
                        kp += z[kk] * z[kk];
                        const float qd = sq[d], gd = sg[d];
                        V(0, d) = qd;
                        V(1, d) = z[kk];
                        V(2, d) = gd;
                        V(3, d) = qd;
                        V(4, d) = z[kk];
                        V(5, d) = gd;
                    }
                }
            }
        }
        const float ks = glm_chain_sum(kp, red[0], pr, j);
        if (f_newit) {
            H0 = -sc.logp + 0.5f * ks;
            const mc_u32x4 rs = mc_draw(cfg.seed, chain_id, it, MC_RNG_TAG_SLICE, 0, 0);
            logu = glm_nuts_slice(H0, mc_logf_u01(mc_u01_f32(rs.x)), cfg.slice_mode);
            n = 1;
            depth = 0;
            asum = 0.0;
            nalpha = 0;
            leaves = 0;
            ndiv = 0;
            f_newit = false;
            if (MAXJ > 0) f_newdepth = true;
            else f_itend = true;
        }
    }

    // ---- the next subtree's direction, and 5. the next leaf's first half
    if (f_newdepth) {
        const mc_u32x4 rd = mc_draw(cfg.seed, chain_id, (uint32_t)(cfg.iter_begin + io),
                                    MC_RNG_TAG_DEPTH, (uint32_t)depth, 0);
        dir = (mc_u01_f32(rd.x) < 0.5f) ? 1 : -1;
        k = 0;
        freem = (1u << (MAXJ + 2)) - 1u;
        cand = 0;
        cn = 0;
        f_leaf = true;
    }
    if (f_leaf) {
        const double ve = (double)dir * sc.step_size;
        const float h = (float)(0.5 * ve);
        const float e = (float)ve;
        const int E = dir > 0 ? 3 : 0;
        GLM_FOR_OWNED(D) {
            const float pj = V(E + 1, d) + h * V(E + 2, d);
            V(VR, d) = pj;
            qt[d * 32] = V(E, d) + e * pj;
        }
    }

    if (live && pr == 0) {
        sw[NW_IO * 32] = (uint32_t)io;
        sw[NW_DEPTH * 32] = (uint32_t)depth;
        sw[NW_K * 32] = (uint32_t)k;
        sw[NW_DIR * 32] = (uint32_t)dir;
        sw[NW_N * 32] = (uint32_t)n;
        sw[NW_CAND * 32] = (uint32_t)cand;
        sw[NW_CN * 32] = (uint32_t)cn;
        sw[NW_FREE * 32] = freem;
        sw[NW_NALPHA * 32] = (uint32_t)nalpha;
        sw[NW_LEAVES * 32] = (uint32_t)leaves;
        sw[NW_DIV * 32] = (uint32_t)ndiv;
        sw[NW_H0 * 32] = __float_as_uint(H0);
        glm_nuts_st(sw, NW_LOGU, logu);
        glm_nuts_st(sw, NW_ASUM, asum);
        sw[NW_DONE * 32] = done ? 1u : 0u;
        scal[c] = sc;
    }
    if (pr == 0) lv[j] = done ? 0 : 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        int left = 0;
        for (int i = 0; i < kGlmChains; ++i) left += lv[i];
        cnt[cb] = left;
    }
}

// the chains of a launch that are not done: the sum of the blocks' counts
template <int = 0>
__global__ void k_glm_nuts_left(const int32_t* cnt, int64_t blocks, int32_t* left) {
    int s = 0;
    for (int64_t b = threadIdx.x; b < blocks; b += 64) s += cnt[b];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) *left = s;
}

}  // namespace mc
