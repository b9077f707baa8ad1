"""Plain numpy for the tests of the fused kNN's ranking tiers: no GPU, no library.

The fused kNN ranks candidates on a reduced-precision shadow of the data, keeps the best k1 - 1
entries, evaluates only those exactly and certifies per query, through a hand-derived rounding
bound, that no dropped row belongs to the answer (rp-tree_amd/csrc/knn.hip).  On centred,
well-conditioned data the shadow's order IS the exact order and any bound certifies a cut that was
right anyway.  This module builds inputs on which the shadow really misranks and says, on the CPU,
how far each one pushes the certificate:

  * an EMULATION of every shadow's ranking value (Shadow / CsrShadow).  It is a proxy, not the
    kernel's bits (the dense emulation sums in float64, the kernels in float32 butterflies): it is
    used to prove what the cases are, never to check the kernel;
  * the STATED BOUNDS, restated from the comments of knn.hip (err_dense, tier_bounds, csr_e2,
    csr_emax) and the critical scale of a case: the factor on the additive bound below which the
    certificate would pass although the kept set misses true neighbours.  A bound multiplied by
    less than that factor gives a wrong answer on the case;
  * the CASE BUILDERS: offset sweeps, aligned half-ulp cases (also with the decoys of the wider
    in-kernel retry and with the rows that set max_norm first, last or in the middle), the int8
    tier's one-outlier case.

Tier names: "f32" (f64 rows on their f32 shadow, tier 1), "half" (f64 rows on their IEEE-half shadow,
tier 2), "f32half" (f32 rows on their half shadow, tier 2), "int8" (tier 3), "csr32" (CSR rows on the
(u16, f32) shadow, tier 1), "ell" (CSR rows on the fixed-width half table, tier 2)."""
import itertools
import math

import numpy as np

U = 2.0 ** -24            # unit roundoff of float32
H16 = 2.0 ** -11          # ... of IEEE half
K_BK = 224                # kBK of knn_plan.h: the widest list of the workgroup kernel


# ------------------------------------------------------------------ what the plan keeps
def kept(tier, k, d=128, wave=False):
    """entries the first attempt keeps (k1 - 1 of knn_plan.h).  The int8 tier's margin grows with the
    row length, max(48, k) sqrt(d / 128), and the one-wave kernel keeps at most 47 (up to 4000 candidates
    per query, a forest that has not raised its margin yet)"""
    if tier in ("f32", "csr32"):
        return k + max(6, k // 2)
    if tier in ("half", "f32half", "ell"):
        return k + max(8, k // 2)
    keep = k + int(max(48, k) * (math.sqrt(d / 128.0) if d > 128 else 1.0))
    return min(keep, 47 if wave else K_BK - 1)


def kept_retry(tier, k):
    """entries of the workgroup kernel's wider second attempt (k1_retry - 1; dense tiers only)"""
    k1 = kept(tier, k) + 1
    return min(3 * k1, K_BK) - 1


# ------------------------------------------------------------------ emulation, dense
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _half(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


class Shadow:
    """The dense shadows' ranking value, as a distance estimate, in float64."""

    def __init__(self, tier, X):
        self.tier = tier
        X = np.asarray(X)
        self.f64_data = X.dtype == np.float64
        Xd = X.astype(np.float64)
        self.d = X.shape[1]
        self.xmax = float(np.sqrt((Xd * Xd).sum(1).max()))       # data->max_norm
        if tier == "f32":
            self.Xs = _f32(Xd)
        elif tier in ("half", "f32half"):
            self.Xs = _half(Xd)                                   # f64 -> f32 -> half
        elif tier == "int8":                                      # Sh8: ONE scale
            self.s = float(np.abs(Xd).max()) / 127.0
            self.codes = np.clip(np.rint(Xd / self.s), -127, 127)
            e = Xd - self.s * self.codes
            self.emax = float(np.sqrt((e * e).sum(1).max()))
        else:
            raise ValueError(tier)

    def estimate(self, q, idx=None):
        """Dh of the rows idx (all rows: None) for the query q"""
        q = np.asarray(q, dtype=np.float64)
        sel = slice(None) if idx is None else idx
        if self.tier == "int8":
            g = np.clip(np.rint(256.0 * q / self.s), -32768, 32767)
            I = ((g[None, :] - 256.0 * self.codes[sel]) ** 2).sum(1)
            return self.s / 256.0 * np.sqrt(I)
        df = self.Xs[sel] - _f32(q)[None, :]                      # the query stays f32 on every tier
        return np.sqrt((df * df).sum(1))

    def eq(self, q):
        """|q - (s / 256) g| of the int8 tier"""
        q = np.asarray(q, dtype=np.float64)
        g = np.clip(np.rint(256.0 * q / self.s), -32768, 32767)
        e = q - self.s / 256.0 * g
        return float(np.sqrt((e * e).sum()))


def exact_dense(X, q, idx=None):
    """float64 truth (the differences first: no cancellation)"""
    sel = slice(None) if idx is None else idx
    df = np.asarray(X)[sel].astype(np.float64) - np.asarray(q, dtype=np.float64)[None, :]
    return np.sqrt((df * df).sum(1))


# ------------------------------------------------------------------ emulation, CSR
class Csr:
    """rows with the SAME number m <= 64 of nonzeros each: cols [n][m] strictly ascending, vals [n][m]"""

    def __init__(self, cols, vals, d):
        self.cols = np.ascontiguousarray(cols, dtype=np.int32)
        self.vals = np.ascontiguousarray(vals, dtype=np.float64)
        self.n, self.m = self.vals.shape
        self.d = int(d)
        assert self.m <= 64 and self.cols.shape == self.vals.shape

    def arrays(self):
        """(rowptr, col, val, d): what rptree_amd takes"""
        rowptr = np.arange(self.n + 1, dtype=np.int64) * self.m
        return rowptr, self.cols.reshape(-1).copy(), self.vals.reshape(-1).copy(), self.d

    def dense(self):
        D = np.zeros((self.n, self.d))
        D[np.arange(self.n)[:, None], self.cols] = self.vals
        return D

    def ascending(self):
        return bool((np.diff(self.cols, axis=1) > 0).all()) and int(self.cols.min()) >= 0 and \
            int(self.cols.max()) < self.d


class CsrShadow:
    """The two CSR shadows' ranking value (a SQUARED distance, clamped at 0), in float32 arithmetic
    laid out as the kernels lay it out (sixteen lanes per row, four slots each, butterfly): the part
    of the error that is arithmetic, not input rounding, is what these tiers' bound mostly covers."""

    def __init__(self, tier, csr):
        assert tier in ("csr32", "ell")
        self.tier, self.csr = tier, csr
        self.xmax = float(np.sqrt((csr.vals ** 2).sum(1).max()))
        self.max_rowlen = csr.m
        v = csr.vals
        self.vs = (v.astype(np.float32) if tier == "csr32"
                   else v.astype(np.float32).astype(np.float16).astype(np.float32))

    def estimate2(self, q_dense, idx=None):
        """the float32 squared-distance estimate of the rows idx for a dense-ified query"""
        sel = slice(None) if idx is None else idx
        q32 = np.asarray(q_dense, dtype=np.float64).astype(np.float32)
        x = self.vs[sel]
        qj = q32[self.csr.cols[sel]]
        n, m = x.shape
        pad = (-m) % 64
        if self.tier == "csr32":
            df = x - qj
            term = df * df - qj * qj                               # float32, one rounding per operation
            term = np.pad(term, ((0, 0), (0, pad))).reshape(n, 16, 4)
            s = np.zeros((n, 16), dtype=np.float32)
            for e in range(4):
                s = s + term[:, :, e]
        else:
            x = np.pad(x, ((0, 0), (0, pad))).reshape(n, 16, 4).astype(np.float64)
            qj = np.pad(qj, ((0, 0), (0, pad))).reshape(n, 16, 4).astype(np.float64)
            s = np.zeros((n, 16), dtype=np.float32)
            for e in range(4):                                    # s = fma(x, fma(-2, q, x), s)
                inner = (x[:, :, e] - 2.0 * qj[:, :, e]).astype(np.float32).astype(np.float64)
                s = (x[:, :, e] * inner + s.astype(np.float64)).astype(np.float32)
        for o in (8, 4, 2, 1):
            s = s[:, :o] + s[:, o:2 * o]
        qn2 = np.float32((np.asarray(q_dense, dtype=np.float64) ** 2).sum())
        t = qn2 + s[:, 0]
        return np.maximum(t, np.float32(0)).astype(np.float64)


def exact_csr(csr, q_dense, idx=None):
    sel = slice(None) if idx is None else idx
    D = np.tile(-np.asarray(q_dense, dtype=np.float64), (csr.vals[sel].shape[0], 1))
    rows = np.arange(D.shape[0])[:, None]
    D[rows, csr.cols[sel]] += csr.vals[sel]
    return np.sqrt((D * D).sum(1))


# ------------------------------------------------------------------ the stated bounds (knn.hip)
def err_dense(tier, f64_data, d, xmax, qnorm, F):
    """the refine step's err of the workgroup and the one-wave kernel (the same expression twice)"""
    if tier in ("half", "f32half"):
        err = 1.05 * H16 * xmax + 2.1 * U * qnorm + (d + 2) * U * F + np.sqrt(d) * 3.1e-8
    else:
        err = 2.1 * U * (xmax + qnorm) + (d + 2) * U * F + np.sqrt(d) * 4e-23
    if not f64_data:                       # f32 data: the extra (d + 2) u term
        err = err + (d + 2) * U * (F + err) * 1.01
    return err


def err_int8(f64_data, d, eq, emax, F):
    e8 = (eq + emax) * (1.0 + 1e-12) + 1e-300
    return e8 if f64_data else e8 + (d + 2) * U * F * 1.01


def tier_bounds(tier, f64_data, d, xmax, qnorm, eq=0.0, emax=0.0):
    """(A, Bt, Bf) of TierBounds (the shard kernels): lower(Dh) = (Dh - A - Bt Dh)(1 - Bf)"""
    if tier == "int8":
        A = (eq + emax) * (1.0 + 1e-12) + 1e-300
    elif tier in ("half", "f32half"):
        A = 1.05 * H16 * xmax + 2.1 * U * qnorm + np.sqrt(d) * 3.1e-8
    else:
        A = 2.1 * U * (xmax + qnorm) + np.sqrt(d) * 4e-23
    Bt = 0.0 if tier == "int8" else (d + 2) * U
    Bf = 0.0 if f64_data else (d + 2) * U * 1.01
    return A, Bt, Bf


def csr_e2(max_rowlen, xmax, qn2):
    chain = 4 * ((max_rowlen + 63) // 64) + 5
    return (chain + 8.0) * U * (2.0 * xmax * xmax + 4.0 * qn2) * 1.01 + 1e-37


def csr_emax(max_rowlen, xmax):
    return 1.05 * H16 * xmax + np.sqrt(max_rowlen) * 3.1e-8


# ------------------------------------------------------------------ what a cut does to a query
def cut(est, ex, k, keep):
    """One query: est / ex = estimates and exact distances of its candidates IN CANDIDATE ORDER (ties
    go by position on both).  Returns a dict: the exact and the emulated top k (positions), whether the
    kept set (the first `keep` by estimate) holds every true neighbour, F (the smallest dropped
    estimate, None when nothing is dropped) and dk (the k-th exact distance among the kept)."""
    n = len(est)
    pos = np.arange(n)
    by_est = np.lexsort((pos, est))
    by_ex = np.lexsort((pos, ex))
    kk = min(k, n)
    keep_set = by_est[:keep]
    true_top = by_ex[:kk]
    F = float(est[by_est[keep]]) if n > keep else None
    ex_kept = np.sort(ex[keep_set])
    dk = float(ex_kept[min(kk, len(ex_kept)) - 1])
    missing = np.setdiff1d(true_top, keep_set)
    return {"true_top": true_top, "emu_top": by_est[:kk], "order_differs": not np.array_equal(true_top, by_est[:kk]),
            "missing": missing, "F": F, "dk": dk}


def critical_scale(tier, F, dk, bound):
    """The factor s on the additive bound at which the certificate flips: with the bound x s' for any
    s' < s the cut (F, dk) is certified.  Dense tiers: F - s err > dk.  "csr32": F^2 - s E2 > dk^2,
    bound = E2.  "ell": sqrt(F^2 - s 1.003 E2) - s emax > dk, bound = (E2, emax), by bisection."""
    if tier == "csr32":
        return (F * F - dk * dk) / bound
    if tier == "ell":
        E2, emax = bound
        if not F > dk:
            return 0.0
        lo, hi = 0.0, F * F / (1.003 * E2)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            v = F * F - mid * 1.003 * E2
            if v > 0 and np.sqrt(v) - mid * emax > dk:
                lo = mid
            else:
                hi = mid
        return lo
    return (F - dk) / bound


# ------------------------------------------------------------------ (a) offset sweeps
LADDER = {
    "f32": [2.0 ** 10, 2.0 ** 14, 2.0 ** 17, 2.0 ** 20, 2.0 ** 23],
    "half": [1.0, 8.0, 64.0, 512.0, 2048.0],
    "f32half": [1.0, 8.0, 64.0, 512.0, 2048.0],
    "int8": [0.0, 4.0, 64.0, 1024.0],
    "csr32": [2.0 ** 4, 2.0 ** 8, 2.0 ** 10, 2.0 ** 12, 2.0 ** 14],
    "ell": [1.0, 16.0, 128.0, 1024.0],
}


def offset_sweep(tier, c, n, d, nq, seed, sigma=1.0):
    """X = c + sigma N(0, 1); queries = stored rows plus a small perturbation, every fourth a stored row
    itself.  f32half: float32 rows and queries."""
    rng = np.random.default_rng(seed)
    X = c + sigma * rng.standard_normal((n, d))
    src = rng.choice(n, size=nq, replace=False)
    Q = X[src] + 0.05 * sigma * rng.standard_normal((nq, d))
    Q[::4] = X[src[::4]]
    if tier == "f32half":
        X, Q = X.astype(np.float32), Q.astype(np.float32)
    return np.ascontiguousarray(X), np.ascontiguousarray(Q), src


def offset_sweep_csr(c, n, d, m, nq, seed, sigma=1.0):
    """CSR rows on ONE support of m columns (every second column), the offset on the stored values only"""
    rng = np.random.default_rng(seed)
    cols = np.tile(np.arange(m, dtype=np.int32) * (d // m), (n, 1))
    vals = c + sigma * rng.standard_normal((n, m))
    src = rng.choice(n, size=nq, replace=False)
    qv = vals[src] + 0.05 * sigma * rng.standard_normal((nq, m))
    qv[::4] = vals[src[::4]]
    return Csr(cols, vals, d), Csr(cols[:nq], qv, d), src


def proxy_candidates(src, n, ncand):
    """the host test's stand-in for a forest's candidates: ncand consecutive rows around the source row"""
    return [np.arange(s - ncand // 2, s - ncand // 2 + ncand) % n for s in src]


def sweep_stats(tier, X, Q, k, cands, shadow=None):
    """over the queries: (queries whose emulated top k differs from the exact one while the kept set
    holds every true neighbour, queries whose kept set misses a true neighbour)"""
    csr = tier in ("csr32", "ell")
    sh = shadow or (CsrShadow(tier, X) if csr else Shadow(tier, X))
    Qd = Q.dense() if csr else Q
    differs = misses = 0
    for i, idx in enumerate(cands):
        if csr:
            est, ex = np.sqrt(sh.estimate2(Qd[i], idx)), exact_csr(X, Qd[i], idx)
        else:
            est, ex = sh.estimate(Q[i], idx), exact_dense(X, Q[i], idx)
        c = cut(est, ex, k, kept(tier, k))
        if len(c["missing"]):
            misses += 1
        elif c["order_differs"]:
            differs += 1
    return differs, misses


# ------------------------------------------------------------------ (b), (c) aligned half-ulp cases
def _decoy_patterns(d, ones, count, seed):
    """`count` distinct 0/1 vectors of length d with `ones` ones"""
    out = []
    if math.comb(d, ones) <= 4 * count:                           # few patterns exist: enumerate
        for cmb in itertools.islice(itertools.combinations(range(d), ones), count):
            out.append(cmb)
        if len(out) < count:
            raise ValueError("only %d patterns of %d ones in %d" % (len(out), ones, d))
    else:
        rng = np.random.default_rng(seed)
        seen = set()
        while len(out) < count:
            cmb = tuple(sorted(rng.choice(d, size=ones, replace=False).tolist()))
            if cmb not in seen:
                seen.add(cmb)
                out.append(cmb)
    T = np.zeros((count, d))
    for i, cmb in enumerate(out):
        T[i, list(cmb)] = 1.0
    return T


def _place(block, far, place):
    """block = the rows at the cut (they set max_norm), far = everything else; -> rows, index of block[0]"""
    nf = len(far)
    at = {"first": 0, "last": nf, "middle": nf // 2}[place]
    return np.concatenate([far[:at], block, far[at:]]), at


def aligned_dense(tier, d, k, n, place="first", retry=False, c=1024.0, eta=0.5, seed=0):
    """Let h be half an ulp of the shadow's format in [c, 2c) (c a power of two).
      q            every element c + h - eta h: the f32 shadow rounds it DOWN to c (the half tiers keep
                   the query in f32, where it is exact)
      B (k rows)   every element c + h + eps_i, eps_i = 0.002 (i + 1) h: exact distance (eta h + eps_i)
                   sqrt(d), the k true neighbours; the shadow rounds them UP to c + 2h
      A (decoys)   c + 2h t, t a 0/1 vector with d // 8 ones, representable in the shadow: exact distance
                   h sqrt((d - m)(1 - eta)^2 + m (1 + eta)^2) > B's, shadow distance below B's
      far          n - k - |A| rows of norm ~ 1e-3 sqrt(d): every row but the block is tiny in norm
    |A| = the entries the first attempt keeps, so it keeps only decoys and drops all k true neighbours;
    retry: |A| = the entries of the workgroup kernel's wider second attempt, which then is the attempt
    whose certificate decides.  The block [A, B] is the first rows, the last, or sits in the middle.
    -> dict(X, q, block (index range), ids_B, ids_A, h)."""
    assert tier in ("f32", "half", "f32half")
    h = c * (U if tier == "f32" else H16)
    nA = kept_retry(tier, k) if retry else kept(tier, k)
    m = max(1, d // 8)
    rng = np.random.default_rng(seed)
    A = c + 2.0 * h * _decoy_patterns(d, m, nA, seed)
    B = c + h + (0.002 * h * (np.arange(k) + 1.0))[:, None] * np.ones((k, d))
    far = 1e-3 * rng.standard_normal((n - k - nA, d))
    X, at = _place(np.concatenate([A, B]), far, place)
    q = np.full(d, c + h - eta * h)
    if tier == "f32half":
        X, q = X.astype(np.float32), q.astype(np.float32)
    return {"X": np.ascontiguousarray(X), "q": q, "ids_A": np.arange(at, at + nA),
            "ids_B": np.arange(at + nA, at + nA + k), "h": h, "tier": tier, "k": k, "retry": retry}


def aligned_csr(tier, k, n, place="first", m=16, d=64, c=1024.0, seed=0):
    """CSR rows on one support (the even columns), the query on a column of its own (disjoint support:
    |x - q|^2 = |x|^2 + |q|^2, the query tiny), so a row's distance is its norm and the rounding of the
    stored values moves the squared distance in FIRST order (2 c h per element; a near query would move
    it by h^2 only, far below the float32 arithmetic of the CSR ranking value):
      B (k rows)   every value c + h + eps_i: rounds up to c + 2h
      A (decoys)   c + 2h t, m / 2 + 1 ones: exact norm above B's, shadow norm below B's
      far          rows of norm 1.02 c sqrt(m) (a row of small norm would be the nearest: here the far
                   rows carry max_norm, 2 % above the block's)
    h = half an ulp of float32 ("csr32") or of half ("ell") in [c, 2c)."""
    assert tier in ("csr32", "ell") and m % 2 == 0 and 2 * m <= d
    h = c * (U if tier == "csr32" else H16)
    nA = kept(tier, k)
    rng = np.random.default_rng(seed)
    A = c + 2.0 * h * _decoy_patterns(m, m // 2 + 1, nA, seed)
    B = c + h + (0.004 * h * (np.arange(k) + 1.0))[:, None] * np.ones((k, m))
    far = 1.02 * c + 4.0 * h * rng.integers(0, 64, (n - k - nA, m))
    vals, at = _place(np.concatenate([A, B]), far, place)
    cols = np.tile(np.arange(m, dtype=np.int32) * 2, (n, 1))
    q = Csr(np.array([[1]], dtype=np.int32), np.array([[2.0 ** -10]]), d)
    return {"X": Csr(cols, vals, d), "q": q, "ids_A": np.arange(at, at + nA),
            "ids_B": np.arange(at + nA, at + nA + k), "h": h, "tier": tier, "k": k, "retry": False}


def aligned_report(case):
    """What the emulation says of an aligned case with every row a candidate: the true neighbours the
    first attempt drops, the attempt that decides (its kept entries), F, dk, the stated bound there and
    the critical scale; the relative gap of the float64 truth between the k-th and the (k+1)-th row."""
    tier, k, X = case["tier"], case["k"], case["X"]
    csr = tier in ("csr32", "ell")
    if csr:
        sh = CsrShadow(tier, X)
        qd = case["q"].dense()[0]
        est, ex = np.sqrt(sh.estimate2(qd)), exact_csr(X, qd)
        qn2 = float((qd * qd).sum())
    else:
        sh = Shadow(tier, X)
        est, ex = sh.estimate(case["q"]), exact_dense(X, case["q"])
        qnorm = float(np.sqrt((np.asarray(case["q"], dtype=np.float64) ** 2).sum()))
    first = cut(est, ex, k, kept(tier, k))
    last = cut(est, ex, k, kept_retry(tier, k)) if case["retry"] else first
    F, dk = last["F"], last["dk"]
    if tier == "csr32":
        bound = csr_e2(sh.max_rowlen, sh.xmax, qn2)
    elif tier == "ell":
        bound = (csr_e2(sh.max_rowlen, sh.xmax, qn2), csr_emax(sh.max_rowlen, sh.xmax))
    else:
        bound = err_dense(tier, sh.f64_data, sh.d, sh.xmax, qnorm, F)
    srt = np.sort(ex)
    return {"dropped_first": int(np.isin(case["ids_B"], first["missing"]).sum()),
            "dropped_deciding": int(np.isin(case["ids_B"], last["missing"]).sum()),
            "true_top_is_B": bool(np.array_equal(np.sort(last["true_top"]), case["ids_B"])),
            "F": F, "dk": dk, "bound": bound, "scale": critical_scale(tier, F, dk, bound),
            "gap": float((srt[k] - srt[k - 1]) / srt[k]), "xmax": sh.xmax}


# ------------------------------------------------------------------ (d) int8: one outlier element
def int8_outlier(n, d, nq, seed, outlier=1000.0):
    """N(0, 1) rows, ONE element of one row at `outlier`: it stretches the single scale (s = outlier /
    127), every other element quantises to one of a handful of codes and the integer ranking value ties
    everywhere.  Queries: stored rows moved a little (inside the range), every third far outside it."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    X[n // 3, d // 2] = outlier
    src = rng.choice(n, size=nq, replace=False)
    Q = X[src] + 0.01 * rng.standard_normal((nq, d))
    Q[::3] *= 3.0 * outlier
    return np.ascontiguousarray(X), np.ascontiguousarray(Q), src
