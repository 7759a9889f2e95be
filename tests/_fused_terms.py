"""Fused distribution terms (test helper): a case table that names, per case,
the operands, the evaluation path of csrc/eval.h eval_term the term must take
and the plan csrc/program.hip must give it; a builder over the raw C-ABI
(mc_program_create_affine); the closed-form float64 reference; derived
float32 error bounds; and a float32 restatement with mutations.

Path labels: su0 .. su11 (strided_uscale<DIST, VK, LK>, the MC_SU codes),
strided_generic, seg_normal_pv0 / seg_normal_pv1 (seg_normal_uscale<WPC, PV>)
and seg_generic.  path_of() restates eval_term's dispatch in Python; the JIT's
pruning defines (jit.hip fused_paths) are checked against it, not against
jit.hip.

Reference: the float64 formulas of mlx_mcmc_amd/distributions.py's docstring
on the float32 inputs, transforms and the affine loc in float64 too, the VJPs
of eval.h's comments (elem_normal .. elem_identity, xf_chain), the gammaln
normaliser a value without gradient, no cotangent through a -inf branch.

Bounds (bounds()): as tests/_ragged.py's.  A float32 sum of terms, each
carrying c roundings of its own, summed through at most d additions, is within
gamma(d + c) * sum |parts| of the exact sum, gamma(k) = k U / (1 - k U), where
a term that is itself a difference counts by the magnitudes of its parts.
  c: C_ROUND per distribution and quantity, each rounding written out there
     (a <= 1 ulp unit counts 2 U: division, reciprocal; device logf / expf
     <= 2 ulp, the figure of eval.h's comment, tests/_expr_ops.py
     DOCUMENTED_ULP and tests/test_gpu_transform.py: 4 U).
  d: the serial length of a thread ceil(n / (64 wpc)) (a wave task: 64
     threads), or of a lane's runs in the segment tiles, plus the lane
     butterfly (6), the waves (wpc) and, for log p, the terms; for a vector
     element the contributions it receives; for a segment's parameter its
     longest virtual run plus the pieces combined.
  An operand that reaches the formula with an error of its own (a transformed
  parameter: 4 U |y|; an affine loc: its two operations and the slope's
  transform) adds the change of every output under that error, evaluated on
  the reference by a central perturbation (first order).
Nothing in them is measured on the kernel.
"""
import ctypes
import functools
import math
import zlib

import numpy as np

U = 2.0 ** -24
NORMAL, HALFNORMAL, EXPONENTIAL, GAMMA, BETA, IDENTITY = range(6)
DIST_NAMES = ["Normal", "HalfNormal", "Exponential", "Gamma", "Beta", "Identity"]
PV_, PL_, PS_, PLP_ = 1, 2, 4, 8      # pass-mask bits (csrc/internal.h PASS_*)
HALF_LOG_2PI = 0.91893853320467274178
LOG2 = 0.69314718055994530942
C0 = {NORMAL: -HALF_LOG_2PI, HALFNORMAL: LOG2 - HALF_LOG_2PI}
NPOINTS = 16


# --------------------------------------------------------------------------
# operands, terms, cases
# --------------------------------------------------------------------------
class Op:
    """kind: const | ps | data | pvec | gather; off: parameter offset; val: the
    constant or the data array; idx: the gather index; xf: None | exp | log."""

    def __init__(self, kind, off=0, val=None, idx=None, xf=None):
        self.kind, self.off, self.val, self.xf = kind, off, val, xf
        self.idx = None if idx is None else np.asarray(idx, np.int32)

    @property
    def param(self):
        return self.kind in ("ps", "pvec", "gather")

    @property
    def vec(self):
        return self.kind in ("data", "pvec", "gather")

    def injective(self):
        return self.kind != "gather" or len(np.unique(self.idx)) == len(self.idx)


def K(v):
    return Op("const", val=float(np.float32(v)))


def PS(off, xf=None):
    return Op("ps", off, xf=xf)


def DATA(a):
    return Op("data", val=np.asarray(a, np.float32))


def PVEC(off, xf=None):
    return Op("pvec", off, xf=xf)


def GATHER(off, idx, xf=None):
    return Op("gather", off, idx=idx, xf=xf)


class Term:
    def __init__(self, dist, n, value, loc=None, scale=None, weight=1.0, slope=None, x=None):
        self.dist, self.n, self.weight = dist, int(n), float(weight)
        self.value, self.loc, self.scale, self.slope, self.x = value, loc, scale, slope, x

    @property
    def ops(self):
        return [self.value, self.loc, self.scale]

    @property
    def affine(self):
        return self.slope is not None

    def primary(self):
        for a, o in enumerate(self.ops):
            if o is not None and o.kind == "gather" and not o.injective():
                return a
        return -1


class Plan:
    """What program.hip must plan for one term, in evaluation order."""

    def __init__(self, primary=-1, npass=1, masks=None, task=False, split=False, sync=0):
        self.primary, self.npass, self.masks = primary, npass, masks
        self.task, self.split, self.sync = task, split, sync


class Case:
    def __init__(self, name, D, terms, path, plans=None, wpc=1, attrs=(), edge=None, order=None):
        self.name, self.D, self.terms, self.path, self.wpc = name, D, terms, path, wpc
        self.plans = plans or [Plan() for _ in terms]
        self.attrs = set(attrs)
        self.edge = edge            # (parameter index, value outside the support)
        self.order = order or list(range(len(terms)))   # evaluation order of the terms
        self.expr_param = None      # the JIT variant: -0.5 x^2 over this extra parameter

    def with_expr(self):
        c = Case(self.name + "+expr", self.D + 1, self.terms, self.path, self.plans, self.wpc,
                 self.attrs, self.edge, self.order)
        c.expr_param = self.D
        return c

    def n_param_operands(self):
        t = self.terms[0]
        return sum(1 for o in t.ops + [t.slope, t.x] if o is not None and o.param)


def default_masks(term):
    m = PLP_
    for a, o in enumerate(term.ops):
        if o is not None and o.param:
            m |= 1 << a
    if term.affine and ((term.slope.param) or term.x.param):
        m |= PL_
    return m


# --------------------------------------------------------------------------
# eval_term's dispatch, restated
# --------------------------------------------------------------------------
def _fast_kind(o):
    if o is None or o.kind in ("const", "ps"):
        return 0
    if o.xf is not None:
        return -1           # a transformed vector
    return {"data": 1, "pvec": 2}.get(o.kind, -1)


def path_of(term):
    """The label of the path eval_term takes for `term`."""
    normal = term.dist == NORMAL
    moment = term.dist in (NORMAL, HALFNORMAL)
    scale_vec = term.scale is not None and term.scale.vec
    a = term.primary()
    if a < 0:
        fv = _fast_kind(term.value)
        fl = _fast_kind(term.loc) if normal else 0
        if moment and not scale_vec and fv >= 0 and fl >= 0 and not term.affine:
            return "su%d" % (fv * 3 + fl if normal else 9 + fv)
        return "strided_generic"
    other = term.value if a == 1 else term.loc
    fast = (normal and not scale_vec and a <= 1 and other is not None and other.kind == "data"
            and not term.affine and term.ops[a].xf is None)
    return "seg_normal_pv%d" % a if fast else "seg_generic"


def jit_defines(terms):
    """(MC_JIT_PATHS, MC_JIT_SU, MC_JIT_DISTS) a generated build of a program
    with these fused terms must carry."""
    paths = su = dists = 0
    for t in terms:
        p = path_of(t)
        dists |= 1 << t.dist
        if p.startswith("su"):
            su |= 1 << int(p[2:])
        else:
            paths |= {"strided_generic": 1, "seg_normal_pv0": 2, "seg_normal_pv1": 2,
                      "seg_generic": 4}[p]
    return paths, su, dists


# --------------------------------------------------------------------------
# the segment tiling, restated (program.hip build_segments_ops): virtual
# segments (k, start, len) over the term sorted by its primary index
# --------------------------------------------------------------------------
def seg_plan(term, wpc):
    a = term.primary()
    idx = term.ops[a].idx
    perm = np.argsort(idx, kind="stable")
    s = idx[perm]
    starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    lens = np.diff(np.r_[starts, len(s)])
    T = 64 * wpc
    Lt = None if len(starts) >= T else max(1, -(-term.n // T))
    virt, groups = [], []
    for k, st, ln in zip(s[starts], starts, lens):
        pieces = 1 if Lt is None else -(-int(ln) // Lt)
        base, rem = divmod(int(ln), pieces)
        groups.append((int(k), len(virt), pieces))
        for pc in range(pieces):
            pl = base + (1 if pc < rem else 0)
            virt.append((int(k), int(st), pl))
            st += pl
    split = any(g[2] > 1 for g in groups)
    ntiles = -(-len(virt) // 64)
    # the longest serial chain of one lane: its virtual run in each tile of its wave
    serial = 0
    for w in range(wpc):
        serial = max(serial, sum(max(v[2] for v in virt[64 * t:64 * t + 64])
                                 for t in range(w, ntiles, wpc)))
    return {"perm": perm, "virt": virt, "groups": groups, "split": split, "ntiles": ntiles,
            "serial": serial}


# --------------------------------------------------------------------------
# the formulas, in any dtype
# --------------------------------------------------------------------------
def _lgamma(a):
    import torch

    return torch.lgamma(torch.from_numpy(np.asarray(a, np.float64).copy())).numpy()


def elem(dist, v, m, s, dt):
    """Per element: (lp, [dv, dm, ds], mags (lp, dv, dm, ds), in-support mask).
    mags: the summed magnitudes of each quantity's parts."""
    one, half = dt(1.0), dt(0.5)
    with np.errstate(all="ignore"):
        if dist in (NORMAL, HALFNORMAL):
            ok = np.ones(v.shape, bool) if dist == NORMAL else v >= 0
            d = v - m if dist == NORMAL else v
            var = s * s
            logs = np.log(s)
            q = (half * d * d) / var
            lp = (dt(C0[dist]) - logs) - q
            t = d / var
            u1, u2 = d * d / (var * s), one / s
            out = [-t, t if dist == NORMAL else 0 * t, u1 - u2]
            mags = (abs(C0[dist]) + np.abs(logs) + q, np.abs(t), np.abs(t), u1 + u2)
        elif dist == EXPONENTIAL:
            ok = v >= 0
            logr = np.log(s)
            lp = logr - s * v
            out = [-s + 0 * v, 0 * v, one / s - v]
            mags = (np.abs(logr) + np.abs(s * v), np.abs(s) + 0 * v, 0 * v, one / s + np.abs(v))
        elif dist == GAMMA:
            ok = v > 0
            vs = np.where(ok, v, one)
            lv, logb = np.log(vs), np.log(s)
            lga = _lgamma(m).astype(dt)
            lp = ((m * logb - lga) + (m - one) * lv) - s * vs
            out = [(m - one) / vs - s, logb + lv, m / s - vs]
            mags = (np.abs(m * logb) + np.abs(lga) + np.abs((m - one) * lv) + np.abs(s * vs),
                    np.abs((m - one) / vs) + np.abs(s), np.abs(logb) + np.abs(lv),
                    np.abs(m / s) + np.abs(vs))
        elif dist == BETA:
            ok = (v > 0) & (v < 1)
            vs = np.where(ok, v, half)
            lv, l1v = np.log(vs), np.log(one - vs)
            lb = (_lgamma(m) + _lgamma(s) - _lgamma(np.asarray(m, np.float64) + s)).astype(dt)
            lp = ((m - one) * lv + (s - one) * l1v) - lb
            out = [(m - one) / vs - (s - one) / (one - vs), lv, l1v]
            # (1 - v is rounded before its log: an absolute U in l1v, part "1")
            mags = (np.abs((m - one) * lv) + np.abs(s - one) * (np.abs(l1v) + 1) + np.abs(lb),
                    np.abs((m - one) / vs) + np.abs((s - one) / (one - vs)), np.abs(lv),
                    np.abs(l1v) + 1)
        else:
            ok = np.ones(v.shape, bool)
            lp = v
            out = [one + 0 * v, 0 * v, 0 * v]
            mags = (np.abs(v), one + 0 * v, 0 * v, 0 * v)
    lp = np.where(ok, lp, dt(-np.inf))
    out = [np.where(ok, o, dt(0)) for o in out]
    mags = tuple(np.where(ok, np.asarray(x, np.float64), 0.0) for x in mags)
    return lp, out, mags, ok


# Roundings of one element's quantity beyond the additions of the sum it
# enters, in U (lp, dv, dm, ds); the longest chain of any path:
#  Normal / HalfNormal (elem_normal, strided_uscale, finish_moments):
#   lp: logf 4, c0 rounded 1, c0 - logs 1, d 1 (2 squared), d * d 1, s * s 1,
#       the division 2, the subtraction 1, the weight 1                     = 14
#   dv, dm: d 1, s * s 1, 1 / var 2, w * d 1, the product 1 (+ 2 slack for
#       the moment forms' s1 / var, w *, negation)                          = 8
#   ds: d 2, d * d 1, s * s 1, var * s 1, the division 2, 1 / s 2, the
#       subtraction 1, the weight 1, cnt / s 2 (finish_moments)             = 14
#  Exponential: lp: logf 4, r * v 1, the subtraction 1, w 1 (+ 1)            = 8
#   dv: w 1 (+ 1) = 2;  ds: 1 / r 2, the subtraction 1, w 1 (+ 1)            = 5
#  Gamma: lp: logf(b) 4, a * logb 1, lgamma rounded 1, - 1, a - 1 1, logf(v)
#       4, the product 1, + 1, b * v 1, - 1, w 1                            = 17
#   dv: a - 1 1, / 2, - 1, w 1 (+ 1) = 6;  dm: logf 4, + 1, w 1              = 6
#   ds: a / b 2, - 1, w 1 (+ 1)                                              = 5
#  Beta: lp: a - 1 1, logf 4, * 1, + 1, lbeta rounded 1, - 1, w 1 (+ 2)       = 12
#   dv: b - 1 1, 1 - v 1, / 2, - 1, w 1 (+ 1) = 7;  dm, ds: logf 4, w 1 (+ 2) = 7
#  Identity: lp: w 1 (+ 1) = 2;  dv: w (exact for 1) 1
C_ROUND = {NORMAL: (14, 8, 8, 14), HALFNORMAL: (14, 8, 8, 14), EXPONENTIAL: (8, 2, 0, 5),
           GAMMA: (17, 6, 6, 5), BETA: (12, 7, 7, 7), IDENTITY: (2, 1, 0, 0)}
K_XF = 4            # device expf / logf: <= 2 ulp
C_CHAIN = {None: 0, "exp": 1 + K_XF, "log": 2}   # xf_chain: c * y (y's own error) | c / x


def _xf(o, x, dt):
    with np.errstate(all="ignore"):
        return np.exp(x) if o.xf == "exp" else (np.log(x) if o.xf == "log" else x)


def _chain(o, c, x, y):
    with np.errstate(all="ignore"):
        return c * y if o.xf == "exp" else (c / x if o.xf == "log" else c)


def _fetch(o, q, n, dt):
    """(value [n], raw parameter x [n] or None, parameter index [n] or None)."""
    if o is None:
        return np.zeros(n, dt), None, None
    if o.kind == "const":
        return np.full(n, dt(np.float32(o.val))), None, None
    if o.kind == "data":
        return o.val.astype(dt), None, None
    j = (np.full(n, o.off) if o.kind == "ps" else
         (o.off + np.arange(n) if o.kind == "pvec" else o.off + o.idx.astype(np.int64)))
    x = q[j].astype(dt)
    return _xf(o, x, dt), x, j


def term_parts(term, q, dt, bounds=False):
    """One term at q in dtype dt: the weighted per-element log density and the
    cotangent of every parameter operand, [(slot, index [n], c [n])], slot 0 ..
    2 the operands, 3 the affine slope, 4 the affine x.  bounds: also, per
    quantity, (magnitudes [n], sensitivity [n], roundings)."""
    n = term.n
    v, xv, jv = _fetch(term.value, q, n, dt)
    m0, xm, jm = _fetch(term.loc, q, n, dt)
    s, xs, js = _fetch(term.scale, q, n, dt)
    if term.scale is None:
        s = np.ones(n, dt)
    m = m0
    if term.affine:
        ub, xb, jb = _fetch(term.slope, q, n, dt)
        xa, xx, jx = _fetch(term.x, q, n, dt)
        m = m0 + ub * xa
    w = dt(np.float32(term.weight))
    lp, d, mags, ok = elem(term.dist, v, m, s, dt)
    cots = []
    for a, (o, x, y, j) in enumerate(zip(term.ops, (xv, xm, xs), (v, m0, s), (jv, jm, js))):
        if o is not None and o.param:
            cots.append((a, j, _chain(o, w * d[a], x, y)))
    if term.affine:
        cm = w * d[1]
        if term.slope.param:
            cots.append((3, jb, _chain(term.slope, cm * xa, xb, ub)))
        if term.x.param:
            cots.append((4, jx, _chain(term.x, cm * ub, xx, xa)))
    if not bounds:
        return w * lp, cots
    # ---- magnitudes, operand errors, roundings (float64 only) ----------------
    aw = abs(float(w))

    def outputs(vv, mm, ss):
        l, dd, _, _ = elem(term.dist, vv, mm, ss, dt)
        return [np.where(ok, l, 0.0)] + dd

    base = outputs(v, m, s)
    sens = [np.zeros(n) for _ in range(4)]
    deltas = [K_XF * U * np.abs(v) if (term.value is not None and term.value.xf) else None,
              None,
              K_XF * U * np.abs(s) if (term.scale is not None and term.scale.xf) else None]
    dm_ = np.zeros(n)
    if term.loc is not None and term.loc.xf:
        dm_ = dm_ + K_XF * U * np.abs(m0)
    if term.affine:   # ub * xa rounded, the sum rounded, the slope's and x's transforms
        kx = (K_XF if term.slope.xf else 0) + (K_XF if term.x.xf else 0)
        dm_ = dm_ + U * (np.abs(m0) + (2 + kx) * np.abs(ub * xa))
    if np.any(dm_ > 0):
        deltas[1] = dm_
    for a, dl in enumerate(deltas):
        if dl is None:
            continue
        args = [v, m, s]
        dfs = []
        for sg in (1.0, -1.0):
            pert = list(args)
            pert[a] = args[a] + sg * dl
            with np.errstate(all="ignore"):
                po = outputs(*pert)
            dfs.append([np.abs(np.where(np.isfinite(po[k]), po[k], base[k]) - base[k])
                        for k in range(4)])
        # (per operand the larger of the two one-sided changes; summed over operands)
        for k in range(4):
            sens[k] = sens[k] + np.maximum(dfs[0][k], dfs[1][k])
    cr = C_ROUND[term.dist]
    info = {"lp": (aw * mags[0], aw * sens[0], cr[0])}
    for a, j, c in cots:
        if a < 3:
            o = term.ops[a]
            y, x = (v, m0, s)[a], (xv, xm, xs)[a]
            mg, sn, cc = aw * mags[1 + a], aw * sens[1 + a], cr[1 + a] + C_CHAIN[o.xf]
        else:
            o = term.slope if a == 3 else term.x
            y, x = (ub, xa)[a - 3], (xb, xx)[a - 3]
            other = np.abs(xa) if a == 3 else np.abs(ub)
            # cm * xa | cm * ub: one product more, the other factor's transform
            oth = term.x if a == 3 else term.slope
            mg, sn = aw * mags[2] * other, aw * sens[2] * other
            cc = cr[2] + 1 + (K_XF if oth.xf else 0) + C_CHAIN[o.xf]
        with np.errstate(all="ignore"):
            f = np.abs(y) if o.xf == "exp" else (1 / np.abs(x) if o.xf == "log" else 1.0)
        info[a] = (mg * f, sn * f, cc)
    return w * lp, cots, info


def _expr_parts(case, q, dt):
    x = q[case.expr_param].astype(dt) if hasattr(q, "astype") else dt(q[case.expr_param])
    return dt(-0.5) * (x * x), -x        # weight -0.5 on square(x): g = -0.5 * (2 x)


def ref_logp_grad(case, q):
    """The float64 reference at the float32 point q [D]."""
    q = np.asarray(q, np.float32)
    g = np.zeros(case.D)
    lp = 0.0
    for t in case.terms:
        l, cots = term_parts(t, q, np.float64)
        lp += float(np.sum(l))
        for a, j, c in cots:
            np.add.at(g, j, c)
    if case.expr_param is not None:
        l, c = _expr_parts(case, q, np.float64)
        lp += float(l)
        g[case.expr_param] += c
    return lp, g


def _gamma(k):
    return k * U / (1.0 - k * U)


def _depth_scalar(case, ti, term):
    """Additions a broadcast quantity of the term passes through."""
    plan = case.plans[case.order.index(ti)]
    if term.primary() >= 0:
        return seg_plan(term, case.wpc)["serial"] + 6 + case.wpc
    T, W = (64, 1) if plan.task else (64 * case.wpc, case.wpc)
    return -(-term.n // T) + 6 + W


def bounds(case, q, extra_depth=0):
    """(lp_bound, g_bound [D]) of a float32 evaluation at q, derived (module
    docstring).  extra_depth: further additions a broadcast quantity passes
    through (a sliced evaluator: one per slice)."""
    q = np.asarray(q, np.float32)
    D = case.D
    mag, sen, kk, joins = np.zeros(D), np.zeros(D), np.zeros(D), np.zeros(D)
    lp_mag = lp_sen = 0.0
    lp_k = 0
    for ti, t in enumerate(case.terms):
        _, cots, info = term_parts(t, q, np.float64, bounds=True)
        dsc = _depth_scalar(case, ti, t) + extra_depth
        mg, sn, cc = info["lp"]
        lp_mag += float(np.sum(mg))
        lp_sen += float(np.sum(sn))
        lp_k = max(lp_k, dsc + cc)
        a_prim = t.primary()
        sp = seg_plan(t, case.wpc) if a_prim >= 0 else None
        for a, j, c in cots:
            mg, sn, cc = info[a]
            np.add.at(mag, j, mg)
            np.add.at(sen, j, sn)
            o = (t.ops + [t.slope, t.x])[a]
            if o.kind == "ps":
                d = np.full(len(j), dsc)
            elif a == a_prim:      # a run: its longest piece, then the pieces
                dg = {k: max(v[2] for v in sp["virt"][f:f + c_]) + c_ for k, f, c_ in sp["groups"]}
                d = np.array([dg[int(i)] for i in o.idx])
            else:
                d = np.ones(len(j))
            np.maximum.at(kk, j, d + cc)
            joins[np.unique(j)] += 1
    if case.expr_param is not None:     # x * x, the weight
        x = float(q[case.expr_param])
        lp_mag += 0.5 * x * x
        mag[case.expr_param] += abs(x)
        kk[case.expr_param] = max(kk[case.expr_param], 2)
        joins[case.expr_param] += 1
    nt = len(case.terms) + (case.expr_param is not None)
    lp_k += nt + 1
    gb = _gamma(kk + joins) * mag + sen * (1 + _gamma(kk + joins))
    return _gamma(lp_k) * lp_mag + lp_sen * (1 + _gamma(lp_k)), gb


# --------------------------------------------------------------------------
# a float32 restatement per path family, with mutations
# --------------------------------------------------------------------------
F32 = np.float32


def _sum_strided(x, T):
    """Thread tid sums x[tid::T] in order; the T partials pairwise."""
    n = len(x)
    pad = np.zeros(-(-n // T) * T, F32)
    pad[:n] = x
    part = pad.reshape(-1, T)
    acc = np.zeros(T, F32)
    for r in part:
        acc = acc + r
    while len(acc) > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def f32_logp_grad(case, q, drop=None, skip_pass=None, skip_virtual=None):
    """The float32 evaluation restated: strided terms by per-thread partial
    sums, segmented ones by per-virtual-segment sums combined per group.
    Mutations (term 0): drop = an element left out; skip_pass = a pass whose
    cotangents are not deposited; skip_virtual = a virtual segment whose
    partial the split combination leaves out."""
    q = np.asarray(q, F32)
    g = np.zeros(case.D, F32)
    lp = F32(0)
    for ti, t in enumerate(case.terms):
        plan = case.plans[case.order.index(ti)]
        l, cots = term_parts(t, q, F32)
        keep = np.ones(t.n, bool)
        if ti == 0 and drop is not None:
            keep[drop] = False
        masks = plan.masks if plan.masks is not None else [default_masks(t)]
        skipped = 0
        if ti == 0 and skip_pass is not None:
            skipped = masks[skip_pass] & 7
        T = 64 if plan.task else 64 * case.wpc
        a_prim = t.primary()
        if a_prim < 0:
            lp = lp + _sum_strided(np.where(keep, l, F32(0)), T)
        else:
            sp = seg_plan(t, case.wpc)
            ls = np.where(keep, l, F32(0))[sp["perm"]]
            lp = lp + _sum_strided(np.array([np.sum(ls[st:st + ln], dtype=F32)
                                             for _, st, ln in sp["virt"]], F32), T)
        for a, j, c in cots:
            bit = (1 << a) if a < 3 else PL_
            if skipped & bit:
                continue
            c = np.where(keep, c, F32(0)).astype(F32)
            o = (t.ops + [t.slope, t.x])[a]
            if o.kind == "ps":
                g[o.off] += _sum_strided(c, T)
            elif a == a_prim:
                cs = c[sp["perm"]]
                for k, f, cnt in sp["groups"]:
                    acc = F32(0)
                    for vi in range(f, f + cnt):
                        if ti == 0 and skip_virtual == vi:
                            continue
                        _, st, ln = sp["virt"][vi]
                        acc = acc + np.sum(cs[st:st + ln], dtype=F32)
                    g[o.off + k] += acc
            else:
                np.add.at(g, j, c)
    if case.expr_param is not None:
        l, c = _expr_parts(case, q, F32)
        lp = lp + l
        g[case.expr_param] += c
    return lp, g


# --------------------------------------------------------------------------
# points
# --------------------------------------------------------------------------
def _domains(case):
    """Per parameter: 0 real, 1 positive, 2 in (0, 1), 3 above 1."""
    dom = np.zeros(case.D, int)

    def mark(o, n, code):
        if o is None or not o.param:
            return
        j = ([o.off] if o.kind == "ps" else
             (o.off + np.arange(n) if o.kind == "pvec" else o.off + o.idx))
        if o.xf == "exp":
            return
        if o.xf == "log":
            code = 3 if code == 1 else 1
        dom[j] = np.maximum(dom[j], code)

    for t in case.terms:
        pos_value = t.dist in (HALFNORMAL, EXPONENTIAL, GAMMA)
        mark(t.value, t.n, 2 if t.dist == BETA else (1 if pos_value else 0))
        if t.dist in (GAMMA, BETA):
            mark(t.loc, t.n, 1)
        elif t.loc is not None and t.loc.xf == "log":
            mark(t.loc, t.n, 0)
        if t.dist != IDENTITY:
            mark(t.scale, t.n, 1)
        if t.value is not None and t.value.xf == "log" and not pos_value:
            mark(t.value, t.n, 0)
    return dom


def _rng(name, salt=0):
    return np.random.default_rng(zlib.crc32(name.encode()) + salt)


def points(case):
    """[NPOINTS, D] float32 points inside every support; with case.edge, the
    last point has exactly one vector element outside it."""
    rng = _rng(case.name, 1)
    dom = _domains(case)
    D = case.D
    base = np.where(dom == 0, rng.normal(0.0, 1.0, D),
                    np.where(dom == 1, rng.uniform(0.6, 2.0, D),
                             np.where(dom == 2, rng.uniform(0.2, 0.8, D),
                                      rng.uniform(1.5, 4.0, D))))
    pts = np.tile(base, (NPOINTS, 1))
    for k in range(1, NPOINTS):
        z = rng.normal(0.0, 1.0, D)
        pts[k] = np.where(dom == 0, base + 0.3 * z,
                          np.where(dom == 1, base * np.exp(0.25 * z),
                                   np.where(dom == 2, np.clip(base + 0.05 * z, 0.05, 0.95),
                                            1.0 + (base - 1.0) * np.exp(0.25 * z))))
    pts = pts.astype(np.float32)
    if case.edge is not None:
        pts[-1, case.edge[0]] = np.float32(case.edge[1])
    return pts


# --------------------------------------------------------------------------
# the case table
# --------------------------------------------------------------------------
def _data(name, n, kind="real", salt=0):
    rng = _rng(name, 100 + salt)
    if kind == "real":
        return rng.normal(0.5, 1.5, n).astype(np.float32)
    if kind == "pos":
        return rng.uniform(0.5, 2.5, n).astype(np.float32)
    return rng.uniform(0.1, 0.9, n).astype(np.float32)


def _groups(lengths, shuffle=None):
    idx = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    if shuffle is not None:
        idx = idx[np.random.default_rng(shuffle).permutation(len(idx))]
    return idx


WEIGHTS = (1.0, -0.5, 2.0)

# strided_uscale: (code, scale kind, n, weight, wave task, wpc)
_SU_ROWS = [
    (0, "const", 1, 1.0, True, 1), (0, "ps", 1, 2.0, True, 1),
    (1, "const", 63, -0.5, True, 1), (1, "ps", 65, 1.0, False, 1),
    (2, "const", 64, 2.0, False, 1), (2, "ps", 257, 1.0, False, 1),
    (3, "const", 64, 1.0, True, 1), (3, "ps", 65, -0.5, False, 1),
    (4, "const", 257, 2.0, False, 1), (4, "ps", 64, 1.0, True, 1),
    (5, "const", 513, 1.0, False, 4), (5, "ps", 65, 2.0, False, 1),
    (6, "const", 63, -0.5, False, 1), (6, "ps", 16385, 1.0, False, 8),
    (7, "const", 65, 1.0, False, 1), (7, "ps", 513, -0.5, False, 4),
    (8, "const", 257, 1.0, False, 1), (8, "ps", 1, 2.0, False, 1),
    (9, "const", 1, 1.0, True, 1), (9, "ps", 1, -0.5, True, 1),
    (10, "const", 63, 2.0, True, 1), (10, "ps", 257, 1.0, False, 1),
    (11, "const", 65, 1.0, False, 1), (11, "ps", 513, 2.0, False, 4),
]


def _su_case(code, sk, n, w, task, wpc, scale_xf=None, value_xf=None, tag=""):
    name = f"su{code}_{sk}{tag}"
    dist = NORMAL if code < 9 else HALFNORMAL
    vk, lk = (code // 3, code % 3) if code < 9 else (code - 9, 0)
    off = 0
    ops = []
    for slot, k in enumerate((vk, lk)):
        if dist == HALFNORMAL and slot == 1:
            ops.append(None)
            continue
        if k == 0:
            ops.append(PS(off, xf=value_xf if slot == 0 else None))
            off += 1
        elif k == 1:
            ops.append(DATA(_data(name, n, "pos" if dist == HALFNORMAL else "real", slot)))
        else:
            ops.append(PVEC(off))
            off += n
    if sk == "ps":
        sc = PS(off, xf=scale_xf)
        off += 1
    else:
        sc = K(1.3)
    D = max(off, 1)
    t = Term(dist, n, ops[0], ops[1], sc, weight=w)
    attrs = {"scale_" + sk, f"w{w:g}", f"n{n}", f"wpc{wpc}"}
    if task:
        attrs.add("task")
    if scale_xf:
        attrs.add("exp_ps_scale")
    if value_xf:
        attrs.add("log_ps_value")
    return Case(name, D, [t], f"su{code}", [Plan(task=task)], wpc, attrs)


def _seg_lengths(kind):
    if kind == "split":          # G < 64 wpc: runs split into virtual segments
        return [1, 200, 40]
    if kind == "whole70":        # 70 groups: the second tile has 6 valid lanes
        return [1 + (3 * i) % 5 for i in range(70)]
    if kind == "ragged":         # lengths 0 .. 7, some parameters never indexed
        return [i % 8 for i in range(80)]
    if kind == "split513":       # wpc 4
        return [100, 13, 250, 150]
    if kind == "whole16385":     # wpc 8, G >= 512: whole runs
        ln = [27] * 600
        ln[-1] += 16385 - sum(ln)
        return ln
    raise ValueError(kind)


def _seg_normal(pv, kind, sk, w, wpc=1, shuffle=None):
    name = f"seg_normal_pv{pv}_{kind}_{sk}" + ("_unsorted" if shuffle else "")
    lengths = _seg_lengths(kind)
    G = len(lengths)
    idx = _groups(lengths, shuffle)
    n = len(idx)
    y = DATA(_data(name, n))
    th = GATHER(0, idx)
    sc = PS(G) if sk == "ps" else K(0.9)
    t = Term(NORMAL, n, y if pv == 1 else th, th if pv == 1 else y, sc, weight=w)
    split = kind.startswith("split")
    attrs = {"scale_" + sk, f"w{w:g}", kind, f"wpc{wpc}", "split" if split else "whole"}
    if shuffle:
        attrs.add("unsorted")
    return Case(name, G + (sk == "ps"), [t], f"seg_normal_pv{pv}",
                [Plan(primary=1 if pv == 1 else 0, split=split)], wpc, attrs)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for row in _SU_ROWS:
        out.append(_su_case(*row))
    out.append(_su_case(6, "ps", 257, 1.0, False, 1, scale_xf="exp", tag="_exp"))
    out.append(_su_case(1, "ps", 65, 2.0, False, 1, value_xf="log", tag="_logv"))
    # support edge: HalfNormal over a parameter vector, one element below 0
    e = _su_case(11, "ps", 65, 1.0, False, 1, tag="_edge")
    e.edge = (7, -0.25)
    e.attrs.add("edge")
    out.append(e)

    def one(name, D, term, path, plan=None, wpc=1, attrs=(), edge=None):
        a = set(attrs) | {f"w{term.weight:g}", f"n{term.n}", f"wpc{wpc}"}
        if edge is not None:
            a.add("edge")
        out.append(Case(name, D, [term], path, [plan or Plan()], wpc, a, edge))

    d = _data
    # ---- strided_generic --------------------------------------------------
    n = 257
    one("sg_normal_vscale", n + 1, Term(NORMAL, n, PVEC(1), PS(0), DATA(d("a", n, "pos"))),
        "strided_generic", attrs={"normal_vscale"})
    n = 65
    one("sg_halfnormal_vscale", n, Term(HALFNORMAL, n, PVEC(0), None, DATA(d("b", n, "pos")),
                                        weight=2.0), "strided_generic", attrs={"halfnormal_vscale"})
    n = 63
    one("sg_exponential_vrate", n, Term(EXPONENTIAL, n, PVEC(0), None, DATA(d("c", n, "pos"))),
        "strided_generic", attrs={"exponential_vrate"}, edge=(5, -0.5))
    n = 64
    one("sg_gamma_vbeta", n, Term(GAMMA, n, PVEC(0), K(2.5), DATA(d("d", n, "pos")), weight=2.0),
        "strided_generic", attrs={"gamma_vbeta"}, edge=(63, 0.0))
    n = 257
    one("sg_beta_vbeta", n + 1, Term(BETA, n, PVEC(1), PS(0), DATA(d("e", n, "pos"))),
        "strided_generic", attrs={"beta_vbeta", "lg_per_element"}, edge=(1, 0.0))
    n = 65
    one("sg_gamma_shapes_vec", n + 1, Term(GAMMA, n, DATA(d("f", n, "pos")), PVEC(1), PS(0)),
        "strided_generic", attrs={"gamma_lg_per_element"})
    one("sg_beta_shapes_vec", 2 * n, Term(BETA, n, DATA(d("g", n, "unit")), PVEC(0), PVEC(n),
                                          weight=2.0), "strided_generic",
        attrs={"beta_lg_per_element"})
    one("sg_gamma_shapes_ps_task", 2, Term(GAMMA, 64, DATA(d("h", 64, "pos")), PS(0), PS(1)),
        "strided_generic", Plan(task=True), attrs={"gamma_ps_shapes", "task"})
    one("sg_gamma_shapes_ps", 2, Term(GAMMA, 65, DATA(d("h", 65, "pos")), PS(0), PS(1)),
        "strided_generic", attrs={"gamma_ps_shapes"})
    one("sg_beta_shapes_ps", 2, Term(BETA, 513, DATA(d("i", 513, "unit")), PS(0), PS(1),
                                     weight=-0.5), "strided_generic", wpc=4,
        attrs={"beta_ps_shapes"})
    n = 65
    rng = _rng("perm")
    one("sg_normal_gathers", 2 * n + 1,
        Term(NORMAL, n, GATHER(1, rng.permutation(n)), GATHER(1 + n, rng.permutation(n)), PS(0)),
        "strided_generic", Plan(npass=1), attrs={"injective_gathers"})
    n = 257
    one("sg_exp_pvec", n + 1, Term(NORMAL, n, DATA(d("j", n)), PS(0), PVEC(1, xf="exp")),
        "strided_generic", attrs={"exp_pvec"})
    n = 65
    one("sg_log_pvec", n, Term(NORMAL, n, DATA(d("k", n)), PVEC(0, xf="log"), K(0.8), weight=2.0),
        "strided_generic", attrs={"log_pvec"})
    one("sg_exp_gather", n + 1, Term(NORMAL, n, DATA(d("l", n)), PS(0),
                                     GATHER(1, rng.permutation(n), xf="exp")),
        "strided_generic", attrs={"exp_gather"})
    one("sg_log_gather", n, Term(NORMAL, n, DATA(d("m", n)),
                                 GATHER(0, rng.permutation(n), xf="log"), K(1.1), weight=-0.5),
        "strided_generic", attrs={"log_gather"})
    n = 257
    one("sg_affine_data_x", 3, Term(NORMAL, n, DATA(d("n", n)), PS(0), PS(2), slope=PS(1),
                                    x=DATA(d("n", n, salt=1))),
        "strided_generic", attrs={"affine_data_x"})
    n = 65
    one("sg_affine_pvec_x", n + 2, Term(NORMAL, n, DATA(d("o", n)), PS(0), K(0.7), slope=PS(1),
                                        x=PVEC(2), weight=2.0),
        "strided_generic", attrs={"affine_pvec_x"})
    n = 513
    one("sg_affine_exp_slope", 3, Term(NORMAL, n, DATA(d("p", n)), PS(0), PS(2),
                                       slope=PS(1, xf="exp"), x=DATA(d("p", n, salt=1))),
        "strided_generic", wpc=4, attrs={"affine_exp_slope"})
    n = 257
    one("sg_identity_pvec", n, Term(IDENTITY, n, PVEC(0), weight=-0.5), "strided_generic",
        attrs={"identity_pvec"})
    n = 63
    one("sg_identity_exp_pvec", n, Term(IDENTITY, n, PVEC(0, xf="exp"), weight=-0.5),
        "strided_generic", attrs={"identity_exp_pvec"})
    n = 16385
    one("sg_normal_vscale_wpc8", n + 1, Term(NORMAL, n, PVEC(1), PS(0), DATA(d("q", n, "pos"))),
        "strided_generic", wpc=8, attrs={"normal_vscale"})
    n = 65
    one("sg_beta_edge", n, Term(BETA, n, PVEC(0), K(2.0), K(3.5)), "strided_generic",
        attrs={"beta_value_pvec"}, edge=(64, 0.0))
    # ---- seg_normal_uscale ------------------------------------------------
    out.append(_seg_normal(1, "split", "ps", 1.0))
    out.append(_seg_normal(1, "whole70", "const", -0.5))
    out.append(_seg_normal(1, "ragged", "ps", 2.0))
    out.append(_seg_normal(1, "whole70", "ps", 1.0, shuffle=3))
    out.append(_seg_normal(1, "split513", "ps", 1.0, wpc=4))
    out.append(_seg_normal(1, "whole16385", "ps", 1.0, wpc=8))
    out.append(_seg_normal(0, "split", "const", 2.0))
    out.append(_seg_normal(0, "whole70", "ps", 1.0))
    out.append(_seg_normal(0, "ragged", "ps", -0.5, shuffle=5))
    out.append(_seg_normal(0, "split513", "const", 1.0, wpc=4))

    # ---- seg_generic ------------------------------------------------------
    def seg(name, dist, kind, build, primary, attrs, wpc=1, shuffle=None, weight=1.0, D_extra=0,
            npass=1, masks=None):
        lengths = _seg_lengths(kind)
        G = len(lengths)
        idx = _groups(lengths, shuffle)
        n = len(idx)
        t = build(n, G, idx)
        t.weight = weight
        split = kind.startswith("split")
        one(name, G + D_extra, t, "seg_generic",
            Plan(primary=primary, split=split, npass=npass, masks=masks), wpc,
            set(attrs) | {kind, "split" if split else "whole"})

    seg("sx_normal_vscale", NORMAL, "whole70",
        lambda n, G, ix: Term(NORMAL, n, DATA(d("r", n)), GATHER(0, ix), DATA(d("r", n, "pos", 1))),
        1, {"normal_vscale"})
    seg("sx_exponential_rate", EXPONENTIAL, "ragged",
        lambda n, G, ix: Term(EXPONENTIAL, n, DATA(d("s", n, "pos")), None, GATHER(0, ix)),
        2, {"exponential_gathered_rate"}, weight=2.0)
    seg("sx_gamma_alpha", GAMMA, "split",
        lambda n, G, ix: Term(GAMMA, n, DATA(d("t", n, "pos")), GATHER(0, ix), PS(G)),
        1, {"gamma_gathered_alpha"}, D_extra=1)
    seg("sx_gamma_beta", GAMMA, "whole70",
        lambda n, G, ix: Term(GAMMA, n, DATA(d("u", n, "pos")), K(2.0), GATHER(0, ix)),
        2, {"gamma_gathered_beta"}, weight=-0.5)
    seg("sx_beta_alpha", BETA, "whole70",
        lambda n, G, ix: Term(BETA, n, DATA(d("v", n, "unit")), GATHER(0, ix), K(1.5)),
        1, {"beta_gathered_alpha"}, shuffle=9)
    seg("sx_halfnormal_scale", HALFNORMAL, "split513",
        lambda n, G, ix: Term(HALFNORMAL, n, DATA(d("w", n, "pos")), None, GATHER(0, ix)),
        2, {"halfnormal_gathered_scale"}, wpc=4)
    seg("sx_exp_primary_split", NORMAL, "split",
        lambda n, G, ix: Term(NORMAL, n, DATA(d("x", n)), PS(G), GATHER(0, ix, xf="exp")),
        2, {"exp_primary"}, D_extra=1)
    seg("sx_exp_primary_whole", NORMAL, "whole70",
        lambda n, G, ix: Term(NORMAL, n, DATA(d("y", n)), PS(G), GATHER(0, ix, xf="exp")),
        2, {"exp_primary"}, D_extra=1, weight=2.0)
    seg("sx_affine", NORMAL, "whole70",
        lambda n, G, ix: Term(NORMAL, n, DATA(d("z", n)), GATHER(0, ix), PS(G + 1), slope=PS(G),
                              x=DATA(d("z", n, salt=1))),
        1, {"affine_gathered_loc"}, D_extra=2)
    n_u = sum(_seg_lengths("whole70"))
    seg("sx_unsorted_pvec", NORMAL, "whole70",
        lambda n, G, ix: Term(NORMAL, n, PVEC(G + 1), GATHER(0, ix), PS(G)),
        1, {"unsorted_pvec_other"}, D_extra=1 + n_u, shuffle=11)
    seg("sx_sorted_pvec_wpc8", NORMAL, "whole16385",
        lambda n, G, ix: Term(NORMAL, n, PVEC(G + 1), GATHER(0, ix), PS(G)),
        1, {"sorted_pvec_other"}, D_extra=1 + 16385, wpc=8)
    # ---- passes ------------------------------------------------------------
    n = 257     # the random-walk prior: Normal(x[:-1], s).log_prob(x[1:])
    one("pass_random_walk", n + 2, Term(NORMAL, n, PVEC(2), PVEC(1), PS(0)), "su8",
        Plan(npass=2, masks=[PLP_ | PV_ | PS_, PL_]), attrs={"npass2"})
    n = 513
    one("pass_random_walk_wpc4", n + 2, Term(NORMAL, n, PVEC(2), PVEC(1), PS(0), weight=2.0),
        "su8", Plan(npass=2, masks=[PLP_ | PV_ | PS_, PL_]), wpc=4, attrs={"npass2"})
    n = 65      # the tree prior: theta[1:] ~ N(theta[parent], s)
    parent = (np.arange(1, n + 1) - 1) // 8
    one("pass_tree", n + 2, Term(NORMAL, n, PVEC(2), GATHER(1, parent), PS(0)), "seg_generic",
        Plan(primary=1, npass=2, masks=[PLP_ | PV_ | PS_, PL_], split=True),
        attrs={"npass2", "tree", "split"})
    n = 257     # value, loc and scale all over overlapping ranges
    one("pass_three", n + 2, Term(NORMAL, n, PVEC(0), PVEC(1), PVEC(2, xf="exp")),
        "strided_generic", Plan(npass=3, masks=[PLP_ | PV_, PL_, PS_]), attrs={"npass3"})
    # ---- barriers ----------------------------------------------------------
    n = 257
    rev = np.arange(n)[::-1].copy()
    A = Term(NORMAL, n, PVEC(2), PS(0), PS(1))
    B = Term(NORMAL, n, GATHER(2, rev), DATA(d("ba", n)), K(1.2), weight=2.0)
    out.append(Case("barrier_overlap", n + 2, [A, B], "barrier", [Plan(), Plan(sync=1)],
                    attrs={"sync1"}))
    B2 = Term(NORMAL, n, PVEC(2 + n), DATA(d("bb", n)), K(1.2), weight=2.0)
    out.append(Case("barrier_disjoint", 2 * n + 2, [A, B2], "barrier", [Plan(), Plan(sync=0)],
                    attrs={"sync0"}))
    # (a gather's writes count as the whole parameter vector, program.hip
    # "conservative": a barrier even where the ranges are disjoint)
    B3 = Term(NORMAL, n, GATHER(2 + n, rev), DATA(d("bc", n)), K(1.2), weight=2.0)
    out.append(Case("barrier_gather_disjoint", 2 * n + 2, [A, B3], "barrier",
                    [Plan(), Plan(sync=1)], attrs={"sync_conservative"}))
    Tk = Term(NORMAL, 64, DATA(d("bd", 64)), PS(0), PS(1), weight=-0.5)
    out.append(Case("barrier_task_between", n + 2, [A, Tk, B], "barrier",
                    [Plan(), Plan(sync=1), Plan(task=True)], attrs={"sync1", "task_last"},
                    order=[0, 2, 1]))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


def labels():
    return [f"su{k}" for k in range(12)] + ["strided_generic", "seg_normal_pv0",
                                            "seg_normal_pv1", "seg_generic"]


def label_case(label):
    """The single-term case of the label with the most parameter operands (of
    equals the longest, up to 600 elements)."""
    best = None
    for c in cases():
        if c.path == label and len(c.terms) == 1 and c.edge is None and c.terms[0].n <= 600:
            key = (c.n_param_operands(), c.terms[0].n)
            if best is None or key > (best.n_param_operands(), best.terms[0].n):
                best = c
    return best


# The (label, attribute) pairs the table must hold (test_completeness).
REQUIRED = (
    [(f"su{k}", a) for k in range(12) for a in ("scale_const", "scale_ps")]
    + [("su6", "exp_ps_scale"), ("su1", "log_ps_value"), ("su11", "edge")]
    + [("strided_generic", a) for a in (
        "normal_vscale", "halfnormal_vscale", "exponential_vrate", "gamma_vbeta", "beta_vbeta",
        "lg_per_element", "gamma_lg_per_element", "beta_lg_per_element", "gamma_ps_shapes",
        "beta_ps_shapes", "injective_gathers", "exp_pvec", "log_pvec", "exp_gather",
        "log_gather", "affine_data_x", "affine_pvec_x", "affine_exp_slope", "identity_pvec",
        "identity_exp_pvec", "edge", "task", "npass3")]
    + [(f"seg_normal_pv{pv}", a) for pv in (0, 1)
       for a in ("split", "whole70", "ragged", "unsorted", "scale_const", "scale_ps")]
    + [("seg_generic", a) for a in (
        "normal_vscale", "exponential_gathered_rate", "gamma_gathered_alpha",
        "gamma_gathered_beta", "beta_gathered_alpha", "halfnormal_gathered_scale", "exp_primary",
        "split", "whole", "affine_gathered_loc", "unsorted_pvec_other", "npass2", "tree")]
    + [("su8", "npass2"), ("barrier", "sync1"), ("barrier", "sync0"), ("barrier", "task_last")]
    + [(lab, w) for lab, w in (("su1", "w-0.5"), ("su0", "w2"), ("su0", "w1"))]
)
REQUIRED_GEOMETRY = ["n1", "n63", "n64", "n65", "n257", "n513", "n16385", "wpc1", "wpc4", "wpc8",
                     "w1", "w-0.5", "w2", "task"]


# --------------------------------------------------------------------------
# the raw C-ABI builder
# --------------------------------------------------------------------------
class Program:
    """What _engine.logp_grad and _engine.ChainSet use of a program."""

    def __init__(self, handle, D, keep):
        self.handle, self.D, self._keep = handle, D, keep

    def plan(self, t):
        from mlx_mcmc_amd import _lib

        out = (ctypes.c_int32 * 10)()
        _lib.check(_lib.load().mc_debug_term_plan(self.handle, t, out, 10))
        return dict(zip(("dist", "n", "primary", "npass", "pass_masks", "wave_task", "ncomb",
                         "ntiles", "nvirt", "sync_before"), list(out)))

    @property
    def wpc(self):
        from mlx_mcmc_amd import _lib

        return _lib.load().mc_program_waves_per_chain(self.handle)

    def close(self):
        from mlx_mcmc_amd import _lib

        if self.handle is not None:
            _lib.load().mc_program_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass


def build(case, host_only=False):
    """The case's program through mc_program_create_affine (with the JIT
    variant's expression term: mc_program_create_expr)."""
    from mlx_mcmc_amd import _lib

    lib = _lib.load()
    kinds = {"const": _lib.MC_OP_CONST, "ps": _lib.MC_OP_PSCALAR, "data": _lib.MC_OP_DATA,
             "pvec": _lib.MC_OP_PVEC, "gather": _lib.MC_OP_GATHER}
    xfs = {None: _lib.MC_XF_NONE, "exp": _lib.MC_XF_EXP, "log": _lib.MC_XF_LOG}
    data, index = [], []
    nd = ni = 0

    def operand(o):
        nonlocal nd, ni
        c = _lib.McOperand()
        if o is None:
            c.kind = _lib.MC_OP_NONE
            return c
        c.kind = kinds[o.kind]
        c.param_offset = int(o.off)
        c.transform = xfs[o.xf]
        if o.kind == "const":
            c.value = o.val
        elif o.kind == "data":
            c.pool_offset = nd
            data.append(o.val)
            nd += len(o.val)
        elif o.kind == "gather":
            c.pool_offset = ni
            index.append(o.idx)
            ni += len(o.idx)
        return c

    nt = len(case.terms) + (case.expr_param is not None)
    terms = (_lib.McTerm * nt)()
    affs = []
    for k, t in enumerate(case.terms):
        terms[k].dist = t.dist
        terms[k].n = t.n
        terms[k].weight = t.weight
        terms[k].value, terms[k].loc, terms[k].scale = (operand(o) for o in t.ops)
        if t.affine:
            a = _lib.McAffine()
            a.slope, a.x = operand(t.slope), operand(t.x)
            affs.append(a)
            terms[k].affine = len(affs)
    c_affs = (_lib.McAffine * max(1, len(affs)))(*affs)
    d = np.ascontiguousarray(np.concatenate(data) if data else np.zeros(0), np.float32)
    ix = np.ascontiguousarray(np.concatenate(index) if index else np.zeros(0), np.int32)
    dp = d.ctypes.data_as(ctypes.c_void_p) if d.size else None
    ip = ix.ctypes.data_as(ctypes.c_void_p) if ix.size else None
    h = ctypes.c_void_p()
    if host_only:
        lib.mc_debug_program_host_only(1)
    try:
        if case.expr_param is None:
            _lib.check(lib.mc_program_create_affine(terms, nt, c_affs, len(affs), case.D, 0.0,
                                                    dp, d.size, ip, ix.size, ctypes.byref(h)))
        else:
            e = terms[nt - 1]
            e.dist, e.n, e.weight, e.affine = _lib.MC_DIST_EXPR, 1, -0.5, 1
            for o in (e.value, e.loc, e.scale):
                o.kind = _lib.MC_OP_NONE
            nodes = (_lib.McExprNode * 2)()
            nodes[0].op, nodes[0].a, nodes[0].b, nodes[0].c = _lib.MC_EX_LEAF, -1, -1, -1
            nodes[0].leaf = operand(PS(case.expr_param))
            nodes[1].op, nodes[1].a, nodes[1].b, nodes[1].c = _lib.MC_EX_SQUARE, 0, -1, -1
            nodes[1].leaf.kind = _lib.MC_OP_NONE
            ex = (_lib.McExpr * 1)()
            ex[0].first, ex[0].count = 0, 2
            _lib.check(lib.mc_program_create_expr(terms, nt, c_affs, len(affs), ex, 1, nodes, 2,
                                                  case.D, 0.0, dp, d.size, ip, ix.size,
                                                  ctypes.byref(h)))
    finally:
        if host_only:
            lib.mc_debug_program_host_only(0)
    return Program(h, case.D, (terms, c_affs, d, ix))


# --------------------------------------------------------------------------
# checks
# --------------------------------------------------------------------------
def check_points(case, q, lp, g, what, need_grad=True, extra_depth=0):
    """Device (lp [P], g [P, D]) at q [P, D] against the reference within
    bounds(); returns the worst error / bound ratios (gradient, log p).  A
    point with a parameter outside the support: log p -inf, that element's
    cotangent exactly 0."""
    q = np.atleast_2d(np.asarray(q, np.float32))
    lp = np.atleast_1d(np.asarray(lp))
    worst_g = worst_lp = 0.0
    fails = []
    for c in range(q.shape[0]):
        rl, rg = ref_logp_grad(case, q[c])
        bl, bg = bounds(case, q[c], extra_depth)
        if np.isneginf(rl):
            if not np.isneginf(lp[c]):
                fails.append(f"point {c}: log p {lp[c]!r}, reference -inf")
        else:
            el = abs(float(lp[c]) - rl)
            worst_lp = max(worst_lp, el / bl)
            if not el <= bl:
                fails.append(f"point {c}: log p {lp[c]!r}, f64 {rl!r}, |err| {el:.3e} > {bl:.3e}")
        if not need_grad:
            continue
        eg = np.abs(np.asarray(g[c], np.float64) - rg)
        exact = bg == 0
        if np.any(eg[exact] != 0):
            fails.append(f"point {c}: {int(np.sum(eg[exact] != 0))} entries not exactly "
                         f"their reference (bound 0)")
        worst_g = max(worst_g, float(np.max(np.where(exact, 0.0, eg / np.maximum(bg, 1e-300)))))
        bad = np.nonzero(~(eg <= bg))[0]
        if bad.size:
            j = int(bad[np.argmax(eg[bad] / np.maximum(bg[bad], 1e-300))])
            fails.append(f"point {c}: g[{j}] = {g[c][j]!r}, f64 {rg[j]!r}, |err| {eg[j]:.3e} > "
                         f"bound {bg[j]:.3e} ({bad.size} entries out)")
    print(f"{what} [{case.path}]: worst |err| / bound: gradient {worst_g:.3f}, log p {worst_lp:.3f}")
    assert not fails, f"{what}: " + "; ".join(fails[:6])
    return worst_g, worst_lp


def within(case, q, lp, g):
    """Is (lp, g) within bounds() of the reference at q?  (the mutation tests)"""
    rl, rg = ref_logp_grad(case, q)
    bl, bg = bounds(case, q)
    ok_lp = (np.isneginf(rl) and np.isneginf(lp)) or abs(float(lp) - rl) <= bl
    return bool(ok_lp and np.all(np.abs(np.asarray(g, np.float64) - rg) <= bg))


def hmc_step_size(case, q0, L=2, trials=8, tol=1e-3):
    """A leapfrog step at which the float64 restatement's energy error over L
    steps stays below tol for `trials` momentum draws (so that every proposal
    is accepted up to that probability): halved from 1e-2 until it holds."""
    rng = _rng(case.name, 7)
    ps = rng.normal(0.0, 1.0, (trials, case.D))
    eps = 1e-2
    while eps > 1e-7:
        worst = 0.0
        for p0 in ps:
            q = np.asarray(q0, np.float64).copy()
            lp0, g = ref_logp_grad(case, q.astype(np.float32))
            p = p0.copy()
            for _ in range(L):
                p = p + 0.5 * eps * g
                q = q + eps * p
                lp1, g = _ref64_at(case, q)
                p = p + 0.5 * eps * g
            dh = (lp1 - 0.5 * p @ p) - (lp0 - 0.5 * p0 @ p0)
            worst = max(worst, abs(dh) if np.isfinite(dh) else np.inf)
        if worst <= tol:
            return eps
        eps *= 0.5
    raise AssertionError(f"{case.name}: no step size found")


def _ref64_at(case, q64):
    """The reference at a float64 point (the restated leapfrog only)."""
    g = np.zeros(case.D)
    lp = 0.0
    for t in case.terms:
        l, cots = term_parts(t, q64, np.float64)
        lp += float(np.sum(l))
        for a, j, c in cots:
            np.add.at(g, j, c)
    if case.expr_param is not None:
        l, c = _expr_parts(case, q64, np.float64)
        lp += float(l)
        g[case.expr_param] += c
    return lp, g


# --------------------------------------------------------------------------
# torch float64 autograd of the same formulas (test_fused_terms_reference.py)
# --------------------------------------------------------------------------
def torch_logp_grad(case, q):
    import torch

    qt = torch.tensor(np.asarray(q, np.float32).astype(np.float64), requires_grad=True)
    f64 = torch.float64

    def fetch(o, n):
        if o is None:
            return None
        if o.kind == "const":
            return torch.full((n,), float(np.float32(o.val)), dtype=f64)
        if o.kind == "data":
            return torch.tensor(o.val.astype(np.float64))
        if o.kind == "ps":
            x = qt[o.off].expand(n)
        elif o.kind == "pvec":
            x = qt[o.off:o.off + n]
        else:
            x = qt[torch.tensor(o.off + o.idx.astype(np.int64))]
        return torch.exp(x) if o.xf == "exp" else (torch.log(x) if o.xf == "log" else x)

    total = torch.zeros((), dtype=f64)
    ninf = torch.tensor(-math.inf, dtype=f64)
    for t in case.terms:
        n = t.n
        v, m, s = fetch(t.value, n), fetch(t.loc, n), fetch(t.scale, n)
        if t.affine:
            m = m + fetch(t.slope, n) * fetch(t.x, n)
        if t.dist == NORMAL:
            lp = C0[NORMAL] - torch.log(s) - 0.5 * (v - m) ** 2 / s ** 2
        elif t.dist == HALFNORMAL:
            lp = torch.where(v >= 0, C0[HALFNORMAL] - torch.log(s) - 0.5 * v ** 2 / s ** 2, ninf)
        elif t.dist == EXPONENTIAL:
            lp = torch.where(v >= 0, torch.log(s) - s * v, ninf)
        elif t.dist == GAMMA:
            ok = v > 0
            vs = torch.where(ok, v, torch.ones_like(v))
            lp = torch.where(ok, m * torch.log(s) - torch.lgamma(m).detach()
                             + (m - 1) * torch.log(vs) - s * vs, ninf)
        elif t.dist == BETA:
            ok = (v > 0) & (v < 1)
            vs = torch.where(ok, v, torch.full_like(v, 0.5))
            lb = (torch.lgamma(m) + torch.lgamma(s) - torch.lgamma(m + s)).detach()
            lp = torch.where(ok, (m - 1) * torch.log(vs) + (s - 1) * torch.log(1 - vs) - lb, ninf)
        else:
            lp = v
        total = total + float(np.float32(t.weight)) * lp.sum()
    if case.expr_param is not None:
        total = total - 0.5 * qt[case.expr_param] ** 2
    if not total.requires_grad:     # a term without parameters
        return float(total), np.zeros(case.D)
    (g,) = torch.autograd.grad(total, qt, allow_unused=True)
    return float(total.detach()), (np.zeros(case.D) if g is None else g.numpy())
