"""The fp32 engine's triangular solves in plain NumPy: the host reference of its refinement, a restatement of its block solves, and
descriptors of single ``rowdot_kernel`` / ``coldot_kernel`` launches with what such a launch must do to memory (which entries it owns,
which elements it reads, the panel-major address rule, the long-double value and forward bound of every owned entry).  Shared by
tests/test_hip_f32_refinement.py, tests/test_hip_solve_kernels.py (GPU) and tests/test_f32_solves_host.py; nothing here needs a GPU.
The sentinels, ``UNIT``, ``NE`` and the bit views are those of tests/tile_cases.py.

The refinement (csrc/sigp_f32.inc): x_0 = L^-T L^-1 b in fp32, then k times  r = b - K~ x  in fp64,  x += L^-T L^-1 fp32(r)  with the sum
in fp64.  The reference does the same with LAPACK's fp32 ``potrf`` of ``K~.astype(float32)``, fp32 substitution both ways and the residual
in long double.
"""
import collections
import functools

import numpy as np
from scipy.linalg import cholesky, solve_triangular
from scipy.linalg.lapack import strtri

import hp_reference as H
import tile_cases as TC
from oracle import gp_oracle as O

LD = H.LD
UNIT, NPT, BITS, NE, SENTINEL = TC.UNIT, TC.NPT, TC.BITS, TC.NE, TC.SENTINEL
NB, TS_BS, TS_RHS = 128, 2048, 4                 # csrc/kernels_misc.hpp
BOUND = 16.0                                     # "ratio to LAPACK on the same matrix" (tests/test_hip_conditioning.py)
D, SEED = 8, 5000
ELL = float(np.sqrt(D))
KINDS = ("rbf", "matern52")
LEVELS = (1e-1, 1e-3)
# n: the smallest order at which a path of the block solves first exists (T = n_pad / 128 tiles)
#   300   T = 3   one big block, no update launches (control)
#   2400  T = 19  a second big block of three tiles: ragged pair of trtri_levels at level 2; forward update, coldot with c0 = 2048
#   2600  T = 21  ragged pair at level 4
#   4100  T = 33  three big blocks, the last a single tile: coldot with c0 = 4096, kb = 128
SIZES = (300, 2400, 2600, 4100)
RIDES = (0, 2)
STEPS = 3
REFINE_CASES = [(kind, n, level) for kind in KINDS for n in SIZES for level in LEVELS]


def n_pad(n):
    return (n + NB - 1) // NB * NB


@functools.lru_cache(maxsize=None)
def problem(n, m=2):
    """(X, y, Xs) of tests' fp32 solve cases: O.synthetic_problem(n, 8, 5000, m)"""
    return O.synthetic_problem(n, D, SEED, m=max(m, 1))


def host_matrix(kind, n, level):
    """K~ by the oracle's covariance function (the host tier; the GPU tier reads the device's own fp64 K~ back)"""
    X = problem(n)[0]
    K = O.cov_unit(kind, X, X, ELL)
    return (K + K.T) / 2 + level * np.eye(n)


# ---- the refinement ---------------------------------------------------------------------------------------------------------------------
def f32_factor(K):
    """LAPACK's fp32 Cholesky factor (lower) of the fp64 matrix rounded to fp32"""
    return cholesky(np.asarray(K).astype(np.float32), lower=True, check_finite=False)


def f32_solve(L32, r):
    """L^-T L^-1 fp32(r) by fp32 substitution, returned in fp64"""
    z = solve_triangular(L32, np.asarray(r, dtype=np.float64).astype(np.float32), lower=True, check_finite=False)
    return solve_triangular(L32, z, lower=True, trans="T", check_finite=False).astype(np.float64)


def residual(Kld, x, b):
    """(b - K~ x in long double, max|r| / max|b|)"""
    r = np.asarray(b, dtype=LD) - Kld @ np.asarray(x, dtype=LD)
    return r, float(np.max(np.abs(r)) / np.max(np.abs(b)))


def residual_floor(K, x, b):
    """the rounding of an fp64 residual of order n:  (n + 2) 2^-53 max(|K~| |x| + |b|) / max|b|"""
    n = len(b)
    return float((n + 2) * H.U * np.max(np.abs(K) @ np.abs(x) + np.abs(b)) / np.max(np.abs(b)))


def reference_sequence(K, b, steps=STEPS, Kld=None):
    """[x_0 .. x_steps] (fp64) and [rho_0 .. rho_steps] of the reference refinement of K~ x = b"""
    Kld = np.asarray(K, dtype=LD) if Kld is None else Kld
    L32 = f32_factor(K)
    x = f32_solve(L32, b)
    xs, rhos = [], []
    for k in range(steps + 1):
        r, rho = residual(Kld, x, b)
        xs.append(x.copy())
        rhos.append(rho)
        if k < steps:
            x = x + f32_solve(L32, r.astype(np.float64))
    return xs, rhos


def exact_solution(K, b, Kld=None):
    """K~^-1 b to fp64 rounding: LAPACK's fp64 solution, refined twice with long-double residuals (each step contracts the error by
    cond(K~) 2^-53 <= 1e-9 on the matrices used here)"""
    Kld = np.asarray(K, dtype=LD) if Kld is None else Kld
    L = np.linalg.cholesky(K)
    sol = lambda r: solve_triangular(L, solve_triangular(L, r, lower=True, check_finite=False), lower=True, trans="T", check_finite=False)   # noqa: E731
    x = np.asarray(sol(np.asarray(b, dtype=np.float64)), dtype=LD)
    for _ in range(2):
        r = np.asarray(b, dtype=LD) - Kld @ x
        x = x + np.asarray(sol(r.astype(np.float64)), dtype=LD)
    return x


def contracts(rhos, floor, factor=10.0):
    """the condition on a case: every step of the reference divides the residual by at least ``factor`` until it is at the floor"""
    return all(rhos[k + 1] <= max(rhos[k] / factor, floor) for k in range(len(rhos) - 1))


# ---- the block solves, restated -----------------------------------------------------------------------------------------------------------
def big_blocks(n):
    return [(c0, min(TS_BS, n - c0)) for c0 in range(0, n, TS_BS)]


def block_inverses(L32):
    """{c0: inverse of the big diagonal block at c0 (lower triangular, fp32, LAPACK strtri)}"""
    out = {}
    for c0, kb in big_blocks(L32.shape[0]):
        inv, info = strtri(np.ascontiguousarray(L32[c0:c0 + kb, c0:c0 + kb]), lower=1)
        assert info == 0
        out[c0] = np.tril(inv)
    return out


def block_forward(L32, inv, Z):
    """X = L^-1 Z (Z [n, nrhs] fp32) as f32_block_forward does it: per big block a product with the inverse diagonal block, then ONE
    update of every row below"""
    Z = np.array(Z, dtype=np.float32)
    X = np.zeros_like(Z)
    for c0, kb in big_blocks(L32.shape[0]):
        X[c0:c0 + kb] = inv[c0] @ Z[c0:c0 + kb]
        Z[c0 + kb:] -= L32[c0 + kb:, c0:c0 + kb] @ X[c0:c0 + kb]
    return X


def block_backward(L32, inv, X):
    """Z = L^-T X as f32_block_backward does it: from the last big block up, a product with the inverse's transpose, then ONE update of
    every row above"""
    X = np.array(X, dtype=np.float32)
    Z = np.zeros_like(X)
    for c0, kb in reversed(big_blocks(L32.shape[0])):
        Z[c0:c0 + kb] = inv[c0].T @ X[c0:c0 + kb]
        X[:c0] -= L32[c0:c0 + kb, :c0].T @ Z[c0:c0 + kb]
    return Z


def substitution(L32, B, which):
    """fp32 LAPACK substitution: which = 0 L^-1 B, 1 L^-T B, 2 L^-T L^-1 B"""
    B = np.asarray(B, dtype=np.float32)
    if which in (0, 2):
        B = solve_triangular(L32, B, lower=True, check_finite=False)
    if which in (1, 2):
        B = solve_triangular(L32, B, lower=True, trans="T", check_finite=False)
    return B


def restatement(L32, inv, B, which):
    B = np.asarray(B, dtype=np.float32)
    if which in (0, 2):
        B = block_forward(L32, inv, B)
    if which in (1, 2):
        B = block_backward(L32, inv, B)
    return B


def hp_substitution(L32, B, which, block=256):
    """the same solves in long double on the fp32 factor's values, blocked so that the inner loops are NumPy products: substitution inside
    a diagonal block of ``block`` rows, one long-double product for the rows outside it"""
    L = np.asarray(L32, dtype=LD)
    X = np.array(B, dtype=LD)
    n = L.shape[0]
    cuts = [(a, min(a + block, n)) for a in range(0, n, block)]
    if which in (0, 2):
        for a, e in cuts:
            X[a:e] = H.forward(L[a:e, a:e], X[a:e])
            X[e:] -= L[e:, a:e] @ X[a:e]
    if which in (1, 2):
        for a, e in reversed(cuts):
            X[a:e] = H.backward(L[a:e, a:e], X[a:e])
            X[:a] -= L[a:e, :a].T @ X[a:e]
    return X


# ---- single launches of rowdot_kernel / coldot_kernel ---------------------------------------------------------------------------------------
# rowdot:  Zout[r][j] (-)= sum_{k in range(j)} (Zin + Zadd)[r][k] Mx[j][k],  j < nrows, r < nrhs;  kmode 0: k in [0, K), 1: [0, j], 2: [j, K)
# coldot:  Zout[r][j]  -=  sum_{k < K} Zin[r][k] Mx[k][j],                   j < ncols, r < nrhs
# Layout of a case (elements; every stride a multiple of 16 bytes), members GAP elements apart:
#     Mx    rowdot [nrows][ld = K + pad]        coldot [K][ld = ncols + pad]
#     Zin   [TS_RHS][ldzin = K + pad]           (Zadd the same shape)
#     Zout  row-major [TS_RHS][ldzout = nrows (ncols) rounded up to 16 bytes + pad], or panel-major [panels][TS_RHS][pm_pw]
GAP = TC.GAP
_ROW_DEFAULTS = collections.OrderedDict(kernel="rowdot", dtype="f32", n=4, K=256, kmode=0, nrhs=1, sub=0, zadd=False, pm_pw=0, j_off=0, members=1, pad=0,
                                        family="normal")
Launch = collections.namedtuple("Launch", list(_ROW_DEFAULTS))       # n: nrows (rowdot) / ncols (coldot)


def launch(**kw):
    d = dict(_ROW_DEFAULTS)
    d.update(kw)
    return Launch(**d)


def launch_id(d):
    parts = [d.kernel, d.dtype, "n%d" % d.n, "K%d" % d.K]
    parts += ["%s=%s" % (k, v) for k, v in d._asdict().items() if k not in ("kernel", "dtype", "n", "K") and v != _ROW_DEFAULTS[k]]
    return "-".join(parts)


def round_up(v, q):
    return (v + q - 1) // q * q


LaunchLayout = collections.namedtuple("LaunchLayout", "ld ldzin ldzout m_rows sM sZi sZo m_elems zin_elems zout_elems panels")


def launch_layout(d):
    ne = NE[d.dtype]
    row = d.kernel == "rowdot"
    m_rows = d.n if row else d.K
    ld = (d.K if row else round_up(d.n, ne)) + d.pad
    ldzin = d.K + d.pad
    if d.pm_pw > 0:
        panels = (d.j_off + d.n - 1) // d.pm_pw + 1
        ldzout, zo = d.pm_pw, panels * TS_RHS * d.pm_pw
    else:
        panels = 0
        ldzout = round_up(d.n, ne) + d.pad
        zo = TS_RHS * ldzout
    sM, sZi, sZo = m_rows * ld + GAP, TS_RHS * ldzin + GAP, zo + GAP
    return LaunchLayout(ld, ldzin, ldzout, m_rows, sM, sZi, sZo, (d.members - 1) * sM + m_rows * ld + GAP, (d.members - 1) * sZi + TS_RHS * ldzin + GAP,
                        (d.members - 1) * sZo + zo + GAP, panels)


def k_range(d, j):
    """[klo, khi) of output entry j"""
    if d.kernel == "coldot" or d.kmode == 0:
        return 0, d.K
    return (0, j + 1) if d.kmode == 1 else (j, d.K)


def out_index(d, L, r, j):
    """element of a member's Zout that holds entry j of right-hand side r: row-major r ldzout + j, or panel-major with g = j_off + j at
    ((g / pm_pw) TS_RHS + r) pm_pw + g % pm_pw"""
    if d.pm_pw > 0:
        g = d.j_off + j
        return ((g // d.pm_pw) * TS_RHS + r) * d.pm_pw + g % d.pm_pw
    return r * L.ldzout + j


def launch_masks(d):
    """dict(own [zout_elems] bool, own_index [members][nrhs][n] int, readM [m_elems], readZ [zin_elems]) -- vectorised; the element loop of
    tests/test_f32_solves_host.py checks it"""
    L = launch_layout(d)
    own = np.zeros(L.zout_elems, bool)
    readM, readZ = np.zeros(L.m_elems, bool), np.zeros(L.zin_elems, bool)
    j = np.arange(d.n)
    idx = np.empty((d.members, d.nrhs, d.n), dtype=np.int64)
    for b in range(d.members):
        for r in range(d.nrhs):
            if d.pm_pw > 0:
                g = d.j_off + j
                idx[b, r] = b * L.sZo + ((g // d.pm_pw) * TS_RHS + r) * d.pm_pw + g % d.pm_pw
            else:
                idx[b, r] = b * L.sZo + r * L.ldzout + j
        Mm = TC.view(readM, b * L.sM, L.m_rows, L.ld)
        Zm = TC.view(readZ, b * L.sZi, TS_RHS, L.ldzin)
        k = np.arange(d.K)
        if d.kernel == "coldot":
            Mm[:, :d.n] = True
            Zm[:d.nrhs, :d.K] = True
        else:
            lo = j[:, None] if d.kmode == 2 else 0
            hi = j[:, None] + 1 if d.kmode == 1 else d.K
            inr = (k[None, :] >= lo) & (k[None, :] < hi)
            Mm[:, :d.K] = inr
            Zm[:d.nrhs, :d.K] = inr.any(axis=0)[None, :]
    own[idx.reshape(-1)] = True
    return dict(own=own, own_index=idx, readM=readM, readZ=readZ)


def launch_operands(d, seed=0):
    """dict(M, Zin, Zadd (or None), Zout: flat arrays of the working type; out0: the prior content of the owned entries [members][nrhs][n]).
    ``normal``: standard normal.  ``cancel``: the prior content equals the product to 1e-6 (sub / coldot), and one k-slice of the
    right-hand sides (the last quarter of K) is 1e-8 of the rest, so a dropped or doubled slice is far outside the bound.  NaN in every element of M
    that no owned entry reads -- that includes, for kmode 1 / 2, the elements that share a 16-byte vector with the first or last one in
    range --, in every element of Zin / Zadd outside the k range any row uses and in right-hand sides >= nrhs; the sentinel in every
    element of Zout the launch does not own (and in the owned ones too where the launch does not read them)."""
    L, t = launch_layout(d), NPT[d.dtype]
    m = launch_masks(d)
    rng = np.random.default_rng([seed, 0 if d.kernel == "rowdot" else 1, d.n, d.K, d.kmode, d.nrhs])
    M = rng.standard_normal(L.m_elems)
    Zin = rng.standard_normal(L.zin_elems)
    Zadd = rng.standard_normal(L.zin_elems) if d.zadd else None
    if d.family == "cancel":
        q = max(NE[d.dtype], d.K // 4)
        for b in range(d.members):
            Zm = TC.view(Zin, b * L.sZi, TS_RHS, L.ldzin)
            Zm[:, d.K - q:d.K] *= 1e-8
            if Zadd is not None:
                TC.view(Zadd, b * L.sZi, TS_RHS, L.ldzin)[:, d.K - q:d.K] *= 1e-8
    M, Zin = M.astype(t), Zin.astype(t)
    Zadd = None if Zadd is None else Zadd.astype(t)
    reads_out = d.kernel == "coldot" or d.sub
    out0 = rng.standard_normal((d.members, d.nrhs, d.n))
    if d.family == "cancel" and reads_out:
        P = launch_products(d, dict(M=M, Zin=Zin, Zadd=Zadd))[0]
        out0 = np.asarray(P, dtype=np.float64) * (1.0 + 1e-6 * out0)
    out0 = out0.astype(t)
    M[~m["readM"]] = np.nan
    Zin[~m["readZ"]] = np.nan
    if Zadd is not None:
        Zadd[~m["readZ"]] = np.nan
    Zout = np.full(L.zout_elems, SENTINEL[d.dtype], dtype=BITS[d.dtype]).view(t)
    if reads_out:
        Zout[m["own_index"].reshape(-1)] = out0.reshape(-1)
    return dict(M=M, Zin=Zin, Zadd=Zadd, Zout=Zout, out0=out0.astype(np.float64))


def launch_products(d, ops):
    """(P, mag) [members][nrhs][n] in long double: sum_k (Zin + Zadd)[r][k] M[..], and sum_k |Zin + Zadd| |M|, over each entry's k range.
    Zin + Zadd is the working-type sum the kernel forms (one rounding, charged to the bound's + 3)."""
    L, t = launch_layout(d), NPT[d.dtype]
    P, mag = np.zeros((d.members, d.nrhs, d.n), dtype=LD), np.zeros((d.members, d.nrhs, d.n), dtype=LD)
    j, k = np.arange(d.n), np.arange(d.K)
    for b in range(d.members):
        Mm = TC.view(ops["M"], b * L.sM, L.m_rows, L.ld)
        Z = TC.view(ops["Zin"], b * L.sZi, TS_RHS, L.ldzin)[:d.nrhs, :d.K]
        if ops.get("Zadd") is not None:
            Z = (Z + TC.view(ops["Zadd"], b * L.sZi, TS_RHS, L.ldzin)[:d.nrhs, :d.K]).astype(t)
        Z = np.nan_to_num(Z.astype(LD), nan=0.0)                      # (columns no row reads carry NaN: they meet zeros of the mask below)
        if d.kernel == "coldot":
            Mt = Mm[:, :d.n].astype(LD)                               # [K][n]
        else:
            lo = j[:, None] if d.kmode == 2 else 0
            hi = j[:, None] + 1 if d.kmode == 1 else d.K
            inr = (k[None, :] >= lo) & (k[None, :] < hi)
            Mt = np.where(inr, Mm[:, :d.K].astype(LD), LD(0)).T      # [K][n], zero outside each row's range
        P[b] = H.hp_matmul(Z, Mt)
        mag[b] = H.hp_matmul(np.abs(Z), np.abs(Mt))
    return P, mag


def launch_reference(d, ops):
    """(ref, bound) [members][nrhs][n]: the long-double value of every owned entry and (K_eff + 3) u (|Zin + Zadd| |M| + |out0|)"""
    P, mag = launch_products(d, ops)
    reads_out = d.kernel == "coldot" or d.sub
    j = np.arange(d.n)
    keff = np.array([k_range(d, int(i))[1] - k_range(d, int(i))[0] for i in j])
    u = LD(UNIT[d.dtype])
    if reads_out:
        ref = ops["out0"].astype(LD) - P
        mag = mag + np.abs(ops["out0"])
    else:
        ref = P
    return ref, (keff[None, None, :] + 3) * u * mag


def launch_judge(d, ops, dev, ref, bound, m=None):
    """(largest |dev - ref| / bound over the owned entries, number of elements outside them whose bits changed)"""
    m = m or launch_masks(d)
    got = dev[m["own_index"].reshape(-1)].reshape(ref.shape).astype(LD)
    e = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(e == 0, LD(0), e / bound)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    keep = ~m["own"]
    bt = BITS[d.dtype]
    moved = int(np.count_nonzero(dev.view(bt)[keep] != ops["Zout"].view(bt)[keep]))
    return float(ratio.max()), moved


def rowdot_cases():
    out = []
    add = lambda **kw: out.append(launch(kernel="rowdot", **kw))   # noqa: E731
    for dt in ("f32", "f64"):
        step, ne = 64 * NE[dt], NE[dt]
        for K in (step, step + ne, 2048):
            add(dtype=dt, n=5, K=K, nrhs=2)
            add(dtype=dt, n=4, K=K, nrhs=3, sub=1, family="cancel", pad=ne)
        # triangular ranges: a partial last workgroup, klo off the step and off the vector boundary (rows 129.. of kmode 2 at K = step + vector)
        for kmode in (1, 2):
            for n in (4, 5, 129):
                add(dtype=dt, n=n, K=round_up(n, ne) if n < 129 else step + ne, kmode=kmode, nrhs=1 + n % 4)
            add(dtype=dt, n=129, K=step + ne, kmode=kmode, nrhs=4, sub=1, family="cancel", pad=ne)
        for nrhs in (1, 2, 3, 4):
            add(dtype=dt, n=9, K=step + ne, nrhs=nrhs, sub=nrhs & 1, zadd=True)
        add(dtype=dt, n=9, K=step, nrhs=2, zadd=True, sub=1, family="cancel")
        # panel-major output: the rows of one launch cross the boundary between panels 0 and 1 (j_off + n > 256), and start in panel 1
        add(dtype=dt, n=12, K=step, nrhs=3, pm_pw=256, j_off=250)
        add(dtype=dt, n=12, K=step, nrhs=2, pm_pw=256, j_off=250, sub=1, zadd=True, kmode=2)
        add(dtype=dt, n=6, K=step, nrhs=4, pm_pw=256, j_off=256)
        add(dtype=dt, n=6, K=step, nrhs=2, members=2, pad=ne)
        add(dtype=dt, n=6, K=step, nrhs=2, members=2, sub=1, kmode=1, pm_pw=256, j_off=254)
    return out


def coldot_cases():
    out = []
    add = lambda **kw: out.append(launch(kernel="coldot", **kw))   # noqa: E731
    for dt in ("f32", "f64"):
        cw, ne = 16 * NE[dt], NE[dt]
        for n in (cw, cw + ne, 2048):
            for K in (16, 128, 200, 2048):
                if n == 2048 and K not in (200, 2048):
                    continue
                add(dtype=dt, n=n, K=K, nrhs=1 + (K // 16 + n) % 4, family="cancel" if K == 200 else "normal", pad=ne if K == 128 else 0)
        for nrhs in (1, 2, 3, 4):
            add(dtype=dt, n=cw + ne, K=200, nrhs=nrhs, pad=ne)
    return out


def refused_launches():
    """(what, Launch, overrides of the call's arguments) the run-and-return entries must answer with SIGP_BAD_ARG"""
    r, c = launch(kernel="rowdot", n=5, K=256, nrhs=2), launch(kernel="coldot", n=64, K=16, nrhs=4)
    full = launch(kernel="rowdot", n=8, K=256, nrhs=4)        # the last element of every buffer (before the gap) is one the launch touches
    return [
        ("rowdot K not a multiple of the vector", r, {"K": 254}),
        ("rowdot ld + 2: 8 bytes", r, {"ld": 258}),
        ("rowdot M one element short", full, {"m_elems": -GAP - 1}),
        ("rowdot Zin one element short", full, {"zin_elems": -GAP - 1}),
        ("rowdot Zout one element short", full, {"zout_elems": -GAP - 1}),
        ("rowdot nrhs = 5", r, {"nrhs": 5}),
        ("rowdot nrhs = 0", r, {"nrhs": 0}),
        ("rowdot kmode = 3", r, {"kmode": 3}),
        ("rowdot one row too many", r, {"n": 6}),
        ("rowdot member stride + 1", launch(kernel="rowdot", n=5, K=256, nrhs=2, members=2), {"sZi": 1}),
        ("rowdot members on one output", launch(kernel="rowdot", n=5, K=256, nrhs=2, members=2), {"sZo": 0}),
        ("rowdot panel past the output", launch(kernel="rowdot", n=5, K=256, nrhs=2, pm_pw=256, j_off=250), {"j_off": 254}),
        ("rowdot triangular range past K", launch(kernel="rowdot", n=8, K=8, kmode=1), {"n": 9}),
        ("coldot column count not a multiple of the vector", c, {"n": 62}),
        ("coldot K one row too many", c, {"K": 17}),
        ("coldot ld + 1", c, {"ld": 65}),
        ("coldot Zout one element short", c, {"zout_elems": -GAP - 1}),
        ("coldot nrhs = 5", c, {"nrhs": 5}),
    ]
