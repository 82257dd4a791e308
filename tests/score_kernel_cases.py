"""Cases, long-double references, a-priori bounds and fp64 emulations of the kernels behind the ARD score gradients, one launch sequence at a
time through the debug library (include/sigp_debug.h):

    sigp_debug_run_ard_pass   ard_center_kernel, ard_grad_partial_kernel<8 | 32, W>, ard_grad_finish_kernel / loo_ard_finish_kernel
    sigp_debug_run_cv_band    cv_band_product_kernel
    sigp_debug_run_predcov    predcov_partial_kernel, predcov_finish_kernel

Shared by tests/test_hip_ard_pass.py, tests/test_hip_score_products.py (GPU) and tests/test_score_kernel_cases_host.py, which puts an fp64 NumPy
emulation of each kernel's formula -- and mutations of it -- through the same judges.  Nothing here needs a GPU.  u = 2^-53 throughout; the
bounds are first order in u (a chain of k roundings counts k u, as in tests/tile_cases.py) and hold no factor fitted to any output.

THE ARD PASS.  Tile t of kbuild_tiles(n_pad) = T (T + 1) covers rows 64 bi .., columns 128 bj .. (tile_coords) and owns the pairs i < n, j < i in
it.  Reference per tile and feature k < d, in long double, on the operands as the device got them and Uc as the device returned it:

    T_k(tile) = sum_ij w_ij h(|U_i - U_j|^2) (uc_ik - uc_jk)^2
    w_ij = P_ij - a_i a_j / sf, sf = q / n (ARD_W_NLML);    w_ij = 2 M_ij + v_i a_j + a_i v_j + 2 eps a_i a_j (ARD_W_LOO)
    h(sq) = exp(-sq / 2) (RBF);    h(sq) = (5/3) (1 + s) exp(-s), s = min(sqrt(5 sq), 1e3) (Matern-5/2)            [ard_h_from_sq]

Bound of |device - T_k(tile)|: the sum over the tile's pairs of four terms, each following one stage of ard_grad_partial_kernel.  With
D_ijk = (uc_ik - uc_jk)^2 and A_ijk = (|uc_ik| + |uc_jk|)^2:

 (i)   rounding of w.  NLML: sf = q / n, a_i / sf, the fma and the product with h -- four roundings, each relative to at most
       m_ij = |P_ij| + |a_i a_j / sf|:  4 u m_ij h D.   LOO: fma(eps2, a_j, v_j), times a_i, fma(v_i, a_j, .), fma(2, M_ij, .), times h, and
       eps2 = 2 eps is exact -- five roundings relative to at most m_ij = 2 |M_ij| + |v_i a_j| + |a_i v_j| + 2 |eps a_i a_j|, and the inner
       ones pass through later ones:  6 u m_ij h D.
 (ii)  error of h:  |w_ij| dh D  with  dh = r h + hp dsq + tiny.
       r: exp_cov is within 2 ulp = 4 u (csrc/kernels_misc.hpp states it, tests/test_hip_covariance_inputs.py section (c) asserts it).  RBF: the
       argument -sq / 2 is exact, r = 4 u.  Matern: 5 sq and the square root leave s with relative error 1.5 u, which exp(-s) turns into 1.5 s u and
       1 + s into at most 1.5 u; then the sum 1 + s, the constant 5/3 and two products: r = (4 + 1.5 s + 1.5 + 4) u, rounded up to (10 + 2 s) u.
       dsq: the squared distance comes in Gram form, n_i + n_j - 2 g, from rows staged RELATIVE TO THE TILE'S LOCAL ORIGIN x_0 = row 64 bi
       (kb_gram_tile).  With y = x - x_0 and dq = d rounded up to 4 terms per sum: staging rounds each coordinate once (relative u, which moves sq by
       at most 2 u (|y_i| + |y_j|)^2), n_i, n_j and g are dq-term fma chains ((dq) u (|y_i|^2 + |y_j|^2 + 2 |y_i| |y_j|) by Cauchy-Schwarz), n_i + n_j
       and the closing fma round once each:  dsq = (dq + 6) u (|y_i| + |y_j|)^2.
       hp bounds |h'| on [sq - dsq, sq]:  h' = -h / 2 (RBF) and h' = -(25/6) exp(-s) (Matern), both largest in size at the interval's lower end.
       tiny = 2^-1073 (times (5/3)(1 + s) for Matern): exp_cov clamps its argument at -746 and rounds into the denormals, where "2 ulp" has no meaning;
       its absolute error there is at most two denormal spacings.
 (iii) the expanded square  u_i^2 rowsum(W)_i + [W (U o U)]_ik - 2 u_i [W U]_ik  of W = w h, each of the three sums a chain of at most 128 terms
       over the tile's columns, plus the squares u_i^2, u_j^2, the product 2 u_i and the two closing fmas (8 more):  (128 + 8) u |W_ij| A_ijk.
       THIS is the term that carries the cancellation: A is of the size of the centred data's spread squared, D of the pair's difference squared.
 (iv)  the fixed-order sums over 4 rows per lane and 16 partial rows per feature: 20 more roundings relative to the same magnitudes:  20 u |W_ij| A_ijk.

Uc:  |Uc - (U - mean)| <= (n + 2) u (|U_ik| + mean_i |U_ik|) on rows < n, features < d (the mean is an n-term sum and a division, the
subtraction rounds once); the padding is exactly zero.  Finish kernels: component k < d equals the sum of the device's partials to
(tiles + 2) u sum |partial|; the noise component equals sn sum_i (P_ii / 2 - a_i^2 / (2 sf)) or sn sum_i (M_ii + v_i a_i + eps a_i^2) to
(n + 8) u of the summed magnitudes (n-term sum, at most 6 roundings per term, the product with sn).

BAND PRODUCT and PREDCOV PARTIALS:  |C_dev - C_ref| <= (K_eff + 2) u (|A| |B|^T), K_eff the tile's k span (tests/tile_cases.py's bound of the same
tile loop).  PREDCOV FINISH:  C_ij = sigma_f (prior_ij + [i == j and noise] sn - sum_s partial_s) on the DEVICE's partials, to (S + 4) u of the
summed magnitudes (S additions, the symmetric part's sum and product, the noise, the difference, the product with sigma_f).
"""
import collections
import functools

import numpy as np

import hp_reference as H

LD = H.LD
U_RND = 2.0 ** -53
SENT_BITS = np.uint64(0x7FF8DEADBEEF0BAD)         # a quiet NaN with a payload nothing computes
TINY = 2.0 ** -1073
C_W = {"nlml": 4, "loo": 6}
C_GRAM, C_SQUARE, C_SUMS, C_NOISE = 6, 8, 20, 8
KERNEL_ID = {"rbf": 1, "matern52": 2}              # SIGP_KERNEL_RBF / SIGP_KERNEL_MATERN52
WSEL = {"nlml": 0, "loo": 1}                       # ARD_W_NLML / ARD_W_LOO
BAND = 384


def sentinels(n):
    return np.full(n, SENT_BITS, dtype=np.uint64).view(np.float64)


def same_bits(a, b):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)))


def kept(a, where):
    """do the entries of ``a`` under the mask still hold the sentinel?"""
    return bool(np.all(np.ascontiguousarray(a).view(np.uint64)[where] == SENT_BITS))


def _ratio(err, bound):
    """largest err / bound; an error where the bound is zero, or a NaN, counts as inf"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max())


# ======================================================================================================================================
# the ARD pass
# ======================================================================================================================================
ArdDesc = collections.namedtuple("ArdDesc", "n_pad n d kern wsel members family")
ARD_SIZES = [(128, 1), (128, 2), (128, 63), (128, 64), (128, 65), (128, 128), (256, 129), (256, 200), (256, 256), (384, 384)]
ARD_DS = [1, 8, 9, 16, 17, 33, 65]
ARD_FAMILIES = ["normal", "offset", "cluster"]


def ard_cases():
    """Every size with every feature count; kernel, weight, member count and feature family rotate so that every d meets both weights and
    both kernels, every family both kernels and both weights, and groups of 3 occur at every n_pad (the host tier checks the cover).  The
    cluster family needs two points: n = 1 takes the normal one."""
    out = []
    for i, (n_pad, n) in enumerate(ARD_SIZES):
        for j, d in enumerate(ARD_DS):
            x = i + j
            fam = ARD_FAMILIES[(i + 2 * j) % 3]
            if n == 1 and fam == "cluster":
                fam = "normal"
            out.append(ArdDesc(n_pad, n, d, ("rbf", "matern52")[x % 2], ("nlml", "loo")[(x // 2 + j // 4) % 2], 3 if x % 3 == 0 else 1, fam))
    return out


def ard_id(c):
    return "npad%d-n%d-d%d-%s-%s-m%d-%s" % c


ArdLayout = collections.namedtuple("ArdLayout", "dp dq ld tiles sU sP sVec sQ sPartial sGrad u_elems m_elems vec_elems q_elems uc_elems partial_elems grad_elems")


def ard_layout(c):
    """gaps between every strided buffer (all strides even where the kernels load 16-byte pairs), and a gap behind the last member"""
    dp, dq, ld = (c.d + 63) // 64 * 64, (c.d + 15) // 16 * 16, c.n_pad + 2
    T = c.n_pad // 128
    tiles = T * (T + 1)
    sU, sP, sVec, sQ, sPartial, sGrad = c.n_pad * dp + 6, c.n_pad * ld + 10, 4 * c.n_pad + 2 + 4, 3, tiles * dp + 5, c.d + 1 + 3
    m = c.members
    return ArdLayout(dp, dq, ld, tiles, sU, sP, sVec, sQ, sPartial, sGrad, m * sU, m * sP, m * sVec, m * sQ, (m - 1) * sU + c.n_pad * dp, m * sPartial,
                     m * sGrad)


def tile_coords(t):
    """(bi, bj) of tile t: the lower-triangle walk of kbuild_mfma_kernel / ard_grad_partial_kernel"""
    u = t >> 1
    k = 0
    while (k + 1) * (k + 2) // 2 <= u:
        k += 1
    return 2 * k + (t & 1), u - k * (k + 1) // 2


def ard_features(c, rng):
    """[n][d] scaled features u = x / l with l = sqrt(d), so that squared distances are O(1) at every d.  normal: N(0,1) / l.  offset: the same
    behind 1e4.  cluster: feature 0 in two clusters at +-3000 with unit scatter, points alternating between them (pairs i - j even share one)."""
    X = rng.standard_normal((c.n, c.d)) / np.sqrt(c.d)
    if c.family == "offset":
        X = X + 1e4
    elif c.family == "cluster":
        X[:, 0] = np.where(np.arange(c.n) % 2 == 0, 3000.0, -3000.0) + rng.standard_normal(c.n)
    return X


@functools.lru_cache(maxsize=8)
def ard_operands(c):
    """flat float64 buffers as the entry takes them: NaN wherever nothing may be read, zeros where the contract wants zeros, sentinels in the
    outputs.  Both weights use the LooArdVecs arena (a at 0, v at 3 n_pad, eps at 4 n_pad): under ARD_W_NLML v and eps hold NaN and q holds
    y^T a; under ARD_W_LOO q holds NaN."""
    L = ard_layout(c)
    rng = np.random.default_rng([20266000, c.n_pad, c.n, c.d, KERNEL_ID[c.kern], WSEL[c.wsel], c.members, ARD_FAMILIES.index(c.family)])
    n, n_pad, d = c.n, c.n_pad, c.d
    U, M = np.full(L.u_elems, np.nan), np.full(L.m_elems, np.nan)
    vec, q = np.full(L.vec_elems, np.nan), np.full(L.q_elems, np.nan)
    ii, jj = np.arange(n)[:, None], np.arange(n)[None, :]
    for m in range(c.members):
        Um = U[m * L.sU:m * L.sU + n_pad * L.dp].reshape(n_pad, L.dp)
        Um[:] = 0.0
        Um[:n, :d] = ard_features(c, rng)
        Mm = M[m * L.sP:m * L.sP + n_pad * L.ld].reshape(n_pad, L.ld)
        Mm[:n, :n] = np.where(jj <= ii, rng.standard_normal((n, n)), np.nan)
        vm = vec[m * L.sVec:(m + 1) * L.sVec]
        vm[:n] = rng.standard_normal(n)
        if c.wsel == "loo":
            vm[3 * n_pad:3 * n_pad + n] = rng.standard_normal(n)
            vm[4 * n_pad] = 0.1 * rng.standard_normal()
        else:
            q[m * L.sQ] = n * rng.uniform(0.5, 1.5)
    sn_m = rng.uniform(0.05, 0.5, c.members)
    ops = dict(U=U, M=M, vec=vec, q=q, sn_m=sn_m, partial=sentinels(L.partial_elems), grad=sentinels(L.grad_elems))
    for v in ops.values():
        v.setflags(write=False)
    return ops


def ard_member(c, ops, m):
    """(single-member descriptor, operands) of member m of a group, its buffers cut out at the group's strides"""
    L = ard_layout(c)
    c1 = c._replace(members=1)
    cut = lambda a, s: np.array(a[m * s:(m + 1) * s])   # noqa: E731
    return c1, dict(U=cut(ops["U"], L.sU), M=cut(ops["M"], L.sP), vec=cut(ops["vec"], L.sVec), q=cut(ops["q"], L.sQ), sn_m=ops["sn_m"][m:m + 1].copy(),
                    partial=cut(ops["partial"], L.sPartial), grad=cut(ops["grad"], L.sGrad))


def _member_views(c, L, ops, m):
    n, n_pad = c.n, c.n_pad
    Um = ops["U"][m * L.sU:m * L.sU + n_pad * L.dp].reshape(n_pad, L.dp)
    Mm = ops["M"][m * L.sP:m * L.sP + n_pad * L.ld].reshape(n_pad, L.ld)
    vm = ops["vec"][m * L.sVec:(m + 1) * L.sVec]
    a, v, eps = vm[:n], vm[3 * n_pad:3 * n_pad + n], vm[4 * n_pad]
    return Um, Mm, a, v, eps, ops["q"][m * L.sQ]


def _h(kern, sq, xp_exp=np.exp):
    if kern == "rbf":
        return xp_exp(-sq / 2)
    s = np.minimum(np.sqrt(5 * sq), 1e3)
    return sq.dtype.type(5) / sq.dtype.type(3) * (1 + s) * xp_exp(-s)


def _weights(c, Mt, a, v, eps, q, I, J, dt):
    """(w, its magnitude m) on rows I x columns J in dtype dt"""
    ai, aj = a[I].astype(dt)[:, None], a[J].astype(dt)[None, :]
    Mt = Mt.astype(dt)
    if c.wsel == "nlml":
        sf = dt(q) / dt(c.n)
        return Mt - ai * aj / sf, np.abs(Mt) + np.abs(ai * aj / sf)
    vi, vj, e = v[I].astype(dt)[:, None], v[J].astype(dt)[None, :], dt(eps)
    return 2 * Mt + vi * aj + ai * vj + 2 * e * ai * aj, 2 * np.abs(Mt) + np.abs(vi * aj) + np.abs(ai * vj) + 2 * np.abs(e * ai * aj)


def _tile_rows_cols(c, t):
    bi, bj = tile_coords(t)
    I = np.arange(64 * bi, min(64 * bi + 64, c.n))
    J = np.arange(128 * bj, min(128 * bj + 128, max(int(I[-1]), 0))) if I.size else np.arange(0)
    return bi, bj, I, J


def ard_reference(c, ops, Uc):
    """per member: dict(ref, bound [tiles][d] long double; S [d]: sum |W| (uc_i - uc_j)^2, the scale of the end-to-end tests)"""
    L = ard_layout(c)
    u, d = LD(U_RND), c.d
    dq4 = (d + 3) // 4 * 4
    out = []
    for m in range(c.members):
        Um, Mm, a, v, eps, q = _member_views(c, L, ops, m)
        Ucm = Uc[m * L.sU:m * L.sU + c.n_pad * L.dp].reshape(c.n_pad, L.dp)
        ref, bound, S = np.zeros((L.tiles, d), dtype=LD), np.zeros((L.tiles, d), dtype=LD), np.zeros(d, dtype=LD)
        for t in range(L.tiles):
            bi, bj, I, J = _tile_rows_cols(c, t)
            if I.size == 0 or J.size == 0:
                continue
            mask = J[None, :] < I[:, None]
            XI, XJ = Um[I, :d].astype(LD), Um[J, :d].astype(LD)
            sq = np.zeros((I.size, J.size), dtype=LD)
            for k in range(d):
                df = XI[:, k][:, None] - XJ[:, k][None, :]
                sq += df * df
            x0 = Um[64 * bi, :d].astype(LD)
            yi, yj = np.sqrt(np.sum((XI - x0) ** 2, axis=1)), np.sqrt(np.sum((XJ - x0) ** 2, axis=1))
            dsq = (dq4 + C_GRAM) * u * (yi[:, None] + yj[None, :]) ** 2
            h = _h(c.kern, sq)
            lo = np.maximum(sq - dsq, 0)
            if c.kern == "rbf":
                rel, hp, tiny = 4 * u, _h("rbf", lo) / 2, LD(TINY)
            else:
                s, slo = np.minimum(np.sqrt(5 * sq), 1e3), np.minimum(np.sqrt(5 * lo), 1e3)
                rel, hp, tiny = (10 + 2 * s) * u, LD(25) / LD(6) * np.exp(-slo), LD(TINY) * LD(5) / LD(3) * (1 + s)
            dh = rel * h + hp * dsq + tiny
            w, mag = _weights(c, Mm[np.ix_(I, J)], a, v, eps, q, I, J, LD)
            w, mag = np.where(mask, w, 0), np.where(mask, mag, 0)
            W, Wabs = w * h, np.abs(w) * h
            e12 = C_W[c.wsel] * u * mag * h + np.abs(w) * dh
            e34 = (128 + C_SQUARE + C_SUMS) * u * Wabs
            UI, UJ = Ucm[I, :d].astype(LD), Ucm[J, :d].astype(LD)
            for k in range(d):
                D = (UI[:, k][:, None] - UJ[:, k][None, :]) ** 2
                A = (np.abs(UI[:, k])[:, None] + np.abs(UJ[:, k])[None, :]) ** 2
                ref[t, k] = np.sum(W * D)
                bound[t, k] = np.sum(e12 * D + e34 * A)
                S[k] += np.sum(Wabs * D)
        out.append(dict(ref=ref, bound=bound, S=S))
    return out


def ard_judge(c, ops, out, refs=None):
    """dict of the largest error / bound of every check, and of what the footprint lost.  ``out``: dict(Uc, partial, grad) as the entry (or
    the emulation) returned them.  Nothing is left out: every partial of every tile and feature, every gradient component."""
    L = ard_layout(c)
    n, n_pad, d, u = c.n, c.n_pad, c.d, LD(U_RND)
    res = dict(uc=0.0, partial=0.0, grad=0.0, noise=0.0, err_over_S=0.0, uc_padding_zero=True, zero_columns=True, n1_zero=True)
    keep_p, keep_g = np.ones(L.partial_elems, bool), np.ones(L.grad_elems, bool)
    refs = refs if refs is not None else ard_reference(c, ops, out["Uc"])     # (the caller may share one: it depends on Uc alone)
    ucz = np.ones(L.uc_elems, bool)
    for m in range(c.members):
        Um, Mm, a, v, eps, q = _member_views(c, L, ops, m)
        Ucm = out["Uc"][m * L.sU:m * L.sU + n_pad * L.dp].reshape(n_pad, L.dp)
        ucz[m * L.sU:m * L.sU + n_pad * L.dp].reshape(n_pad, L.dp)[:n, :d] = False
        X = Um[:n, :d].astype(LD)
        mean = X.sum(axis=0) / n
        res["uc"] = max(res["uc"], _ratio(np.abs(Ucm[:n, :d].astype(LD) - (X - mean)), (n + 2) * u * (np.abs(X) + np.abs(X).sum(axis=0) / n)))
        pm = out["partial"][m * L.sPartial:m * L.sPartial + L.tiles * L.dp].reshape(L.tiles, L.dp)
        keep_p[m * L.sPartial:m * L.sPartial + L.tiles * L.dp].reshape(L.tiles, L.dp)[:, :L.dq] = False
        r = refs[m]
        res["partial"] = max(res["partial"], _ratio(np.abs(pm[:, :d].astype(LD) - r["ref"]), r["bound"]))
        res["zero_columns"] &= bool(np.all(pm[:, d:L.dq] == 0.0))
        if n == 1:
            res["n1_zero"] &= bool(np.all(pm[:, :L.dq] == 0.0))
        gm = out["grad"][m * L.sGrad:m * L.sGrad + d + 1]
        keep_g[m * L.sGrad:m * L.sGrad + d + 1] = False
        psum, pabs = pm[:, :d].astype(LD).sum(axis=0), np.abs(pm[:, :d].astype(LD)).sum(axis=0)
        res["grad"] = max(res["grad"], _ratio(np.abs(gm[:d].astype(LD) - psum), (L.tiles + 2) * u * pabs))
        with np.errstate(divide="ignore", invalid="ignore"):
            eS = np.where(r["S"] > 1e-300, np.abs(gm[:d].astype(LD) - r["ref"].sum(axis=0)) / r["S"], 0)
        res["err_over_S"] = max(res["err_over_S"], float(np.max(np.where(np.isfinite(eS), eS, np.inf))))
        dg, al, sn = np.diagonal(Mm)[:n].astype(LD), a.astype(LD), LD(ops["sn_m"][m])
        if c.wsel == "nlml":
            sf = LD(q) / LD(n)
            terms, mags = dg / 2 - al * al / (2 * sf), np.abs(dg) / 2 + al * al / (2 * sf)
        else:
            vl, e = v.astype(LD), LD(eps)
            terms, mags = dg + vl * al + e * al * al, np.abs(dg) + np.abs(vl * al) + np.abs(e) * al * al
        res["noise"] = max(res["noise"], _ratio(np.abs(LD(gm[d]) - sn * terms.sum()), (n + C_NOISE) * u * sn * mags.sum()))
    res["uc_padding_zero"] = bool(np.all(out["Uc"][ucz] == 0.0))
    res["moved"] = int(np.count_nonzero(~(out["partial"].view(np.uint64)[keep_p] == SENT_BITS))) + int(np.count_nonzero(~(out["grad"].view(np.uint64)[keep_g] == SENT_BITS)))
    res["worst"] = max(res["uc"], res["partial"], res["grad"], res["noise"])
    return res


ARD_MUTATIONS = ("pair_dropped", "mask_le", "rowsum_rows", "previous_a", "matern_cov")


def ard_mutation_applies(c, mut):
    """pair_dropped and rowsum_rows need a pair of non-zero weight: n >= 2, and not the cluster family at n = 2, whose one pair joins the two
    clusters (h = 0 there: every partial is exactly zero whatever is done to W); matern_cov needs the Matern kernel as well; previous_a a group."""
    pair = c.n >= 2 and not (c.family == "cluster" and c.n == 2)
    return {"pair_dropped": pair, "mask_le": True, "rowsum_rows": pair, "previous_a": c.members > 1 and pair, "matern_cov": pair and c.kern == "matern52"}[mut]


def ard_emulate(c, ops, mut=None):
    """The kernels' formulae in fp64 NumPy: ard_center_kernel's mean and subtraction; per tile the Gram form in the tile's local coordinates,
    the masked weight, the expanded square u_i^2 rowsum(W) + W (U o U) - 2 u_i (W U) on the centred features; the finish kernels' sums.
    ``mut``: one of ARD_MUTATIONS -- one owned pair dropped (row min(n, 64) - 1 of tile 0 with the column two to its left, or pair (1, 0));
    the mask j < i taken as j <= i + 1; the row sums paired with rows 4 lq + r instead of lq + 4 r; member m reading member m - 1's a; the
    Matern h replaced by the covariance (1 + s + s^2 / 3) exp(-s)."""
    L = ard_layout(c)
    n, n_pad, d = c.n, c.n_pad, c.d
    Uc, partial, grad = np.zeros(L.uc_elems), np.array(ops["partial"]), np.array(ops["grad"])
    p16 = np.arange(16)
    perm = (np.arange(64) // 16) * 16 + 4 * (p16 % 4)[np.arange(64) % 16] + (p16 // 4)[np.arange(64) % 16]
    for m in range(c.members):
        Um, Mm, a, v, eps, q = _member_views(c, L, ops, m)
        if mut == "previous_a" and m > 0:
            a = _member_views(c, L, ops, m - 1)[2]
        Ucm = Uc[m * L.sU:m * L.sU + n_pad * L.dp].reshape(n_pad, L.dp)
        Ucm[:n, :d] = Um[:n, :d] - Um[:n, :d].sum(axis=0) / n
        pm = partial[m * L.sPartial:m * L.sPartial + L.tiles * L.dp].reshape(L.tiles, L.dp)
        pm[:, :L.dq] = 0.0
        af, vf = np.zeros(n_pad), np.zeros(n_pad)
        af[:n], vf[:n] = a, v
        for t in range(L.tiles):
            bi, bj = tile_coords(t)
            I, J = np.arange(64 * bi, 64 * bi + 64), np.arange(128 * bj, 128 * bj + 128)
            lim = I[:, None] + 1 if mut == "mask_le" else I[:, None] - 1
            mask = (I[:, None] < n) & (J[None, :] <= lim)
            if mut == "pair_dropped" and t == 0:
                i0 = min(n, 64) - 1
                mask[i0, i0 - 2 if i0 >= 2 else 0] = False
            if not mask.any():
                continue
            x0 = Um[64 * bi, :d]
            YI, YJ = Um[I, :d] - x0, Um[J, :d] - x0
            sq = np.maximum((YI * YI).sum(axis=1)[:, None] + (YJ * YJ).sum(axis=1)[None, :] - 2.0 * (YI @ YJ.T), 0.0)
            if mut == "matern_cov" and c.kern == "matern52":
                s = np.minimum(np.sqrt(5 * sq), 1e3)
                h = (1 + s + s * s / 3) * np.exp(-s)
            else:
                h = _h(c.kern, sq)
            with np.errstate(invalid="ignore"):
                w, _ = _weights(c, Mm[np.ix_(I, J)], af, vf, eps, q, I, J, np.float64)
                W = np.where(mask, w * h, 0.0)
            rowsum = W.sum(axis=1)
            if mut == "rowsum_rows":
                rowsum = rowsum[perm]
            UI, UJ = Ucm[I, :L.dq], Ucm[J, :L.dq]
            s_rows = UI * UI * rowsum[:, None] + (W @ (UJ * UJ) - 2.0 * UI * (W @ UJ))
            pm[t, :L.dq] = s_rows.sum(axis=0)
        gm = grad[m * L.sGrad:m * L.sGrad + d + 1]
        gm[:d] = pm[:, :d].sum(axis=0)
        dg = np.diagonal(Mm)[:n]
        gm[d] = ops["sn_m"][m] * (np.sum(0.5 * dg - a * a / (2.0 * (q / n))) if c.wsel == "nlml" else np.sum(dg + a * (eps * a + v)))
    return dict(Uc=Uc, partial=partial, grad=grad)


# ======================================================================================================================================
# the band product
# ======================================================================================================================================
BandDesc = collections.namedtuple("BandDesc", "T members ldpad family")


def band_cases():
    return [BandDesc(T, m, pad, fam) for T in (1, 2, 4) for m, pad in ((1, 0), (2, 16)) for fam in ("normal", "cancel")]


def band_id(c):
    return "T%d-m%d-pad%d-%s" % c


BandLayout = collections.namedtuple("BandLayout", "n_pad ld sP sBand p_elems band_elems")


def band_layout(c):
    n_pad = 128 * c.T
    ld = n_pad + c.ldpad
    sP, sBand = n_pad * ld + 8, n_pad * BAND + 8
    return BandLayout(n_pad, ld, sP, sBand, c.members * sP, c.members * sBand)


def band_window(c, bj):
    """(k0, k1, first band column) of the tiles of block column bj"""
    k0, k1 = max(bj - 1, 0), min(bj + 2, c.T)
    return k0, k1, 128 * (k0 - bj + 1)


def _patterns(rng, K):
    """(p, q) [K] with p_k q_k + p_k+1 q_k+1 = 0 exactly over every aligned pair of columns, in any precision"""
    v, w = rng.standard_normal(K // 2), rng.standard_normal(K // 2)
    return np.repeat(v, 2), np.repeat(w, 2) * np.tile([1.0, -1.0], K // 2)


@functools.lru_cache(maxsize=None)
def band_operands(c):
    """P [n_pad][ld] and the band store [n_pad][384] per member.  normal: standard normal.  cancel: every row of P lies on one pattern over the
    global columns and every row of the band store on a second one, exactly orthogonal over aligned column pairs, plus 1e-6 noise -- a K block
    read from the wrong place is then ~1e6 bounds off.  NaN: the row padding and the member gaps, the band columns 0 .. 127 of block row 0 and
    256 .. 383 of the last block row, which no tile's window reaches.  (Every column of P inside n_pad is inside SOME tile's window, so P
    itself cannot carry NaN there: a tile that read outside its window k0 .. k1 is caught by its value, not by a NaN.)"""
    L = band_layout(c)
    rng = np.random.default_rng([20266100, c.T, c.members, c.ldpad, c.family == "cancel"])
    P, band = np.full(L.p_elems, np.nan), np.full(L.band_elems, np.nan)
    for m in range(c.members):
        Pm = P[m * L.sP:m * L.sP + L.n_pad * L.ld].reshape(L.n_pad, L.ld)
        Bm = band[m * L.sBand:m * L.sBand + L.n_pad * BAND].reshape(L.n_pad, BAND)
        Pm[:, :L.n_pad] = rng.standard_normal((L.n_pad, L.n_pad))
        Bm[:] = rng.standard_normal((L.n_pad, BAND))
        if c.family == "cancel":
            p, q = _patterns(rng, L.n_pad + 256)                       # global column k at index k + 128
            Pm[:, :L.n_pad] = p[128:128 + L.n_pad][None, :] * rng.uniform(0.5, 2.0, L.n_pad)[:, None] + 1e-6 * Pm[:, :L.n_pad]
            for b in range(c.T):
                rows = slice(128 * b, 128 * b + 128)
                Bm[rows] = q[128 * b:128 * b + BAND][None, :] * rng.uniform(0.5, 2.0, 128)[:, None] + 1e-6 * Bm[rows]
        Bm[:128, :128] = np.nan
        Bm[L.n_pad - 128:, 256:] = np.nan
    ops = dict(P=P, band=band, C=sentinels(L.p_elems))
    for v in ops.values():
        v.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=None)
def band_reference(c):
    """per member (ref, bound) [n_pad][n_pad] long double"""
    L, ops, out = band_layout(c), band_operands(c), []
    for m in range(c.members):
        Pm = ops["P"][m * L.sP:m * L.sP + L.n_pad * L.ld].reshape(L.n_pad, L.ld)
        Bm = ops["band"][m * L.sBand:m * L.sBand + L.n_pad * BAND].reshape(L.n_pad, BAND)
        ref, bound = np.zeros((L.n_pad, L.n_pad), dtype=LD), np.zeros((L.n_pad, L.n_pad), dtype=LD)
        for bj in range(c.T):
            k0, k1, c0 = band_window(c, bj)
            K = 128 * (k1 - k0)
            A, B = Pm[:, 128 * k0:128 * k1], Bm[128 * bj:128 * bj + 128, c0:c0 + K]
            ref[:, 128 * bj:128 * bj + 128] = H.hp_matmul(A, B.T)
            bound[:, 128 * bj:128 * bj + 128] = (K + 2) * LD(U_RND) * H.hp_matmul(np.abs(A), np.abs(B).T)
        out.append((ref, bound))
    return out


def band_judge(c, Cdev):
    """(largest error / bound over every entry of every member's C, sentinels lost outside them)"""
    L, worst = band_layout(c), 0.0
    keep = np.ones(L.p_elems, bool)
    for m, (ref, bound) in enumerate(band_reference(c)):
        Cm = Cdev[m * L.sP:m * L.sP + L.n_pad * L.ld].reshape(L.n_pad, L.ld)
        keep[m * L.sP:m * L.sP + L.n_pad * L.ld].reshape(L.n_pad, L.ld)[:, :L.n_pad] = False
        worst = max(worst, _ratio(np.abs(Cm[:, :L.n_pad].astype(LD) - ref), bound))
    return worst, int(np.count_nonzero(~(Cdev.view(np.uint64)[keep] == SENT_BITS)))


def band_emulate(c, mut=None):
    """tile (bi, bj) = rows bi of P against rows bj of the band store over the window, K block by K block in ascending order, in fp64.
    mut = "block_shifted": the first K block of every window reads the band store 128 columns to the right (wrapping at 384)."""
    L, ops = band_layout(c), band_operands(c)
    Cd = np.array(ops["C"])
    for m in range(c.members):
        Pm = ops["P"][m * L.sP:m * L.sP + L.n_pad * L.ld].reshape(L.n_pad, L.ld)
        Bm = ops["band"][m * L.sBand:m * L.sBand + L.n_pad * BAND].reshape(L.n_pad, BAND)
        Cm = Cd[m * L.sP:m * L.sP + L.n_pad * L.ld].reshape(L.n_pad, L.ld)
        for bj in range(c.T):
            k0, k1, c0 = band_window(c, bj)
            acc = np.zeros((L.n_pad, 128))
            for kb in range(k1 - k0):
                cb = c0 + 128 * kb
                if mut == "block_shifted" and kb == 0:
                    cb = (cb + 128) % BAND
                acc += Pm[:, 128 * (k0 + kb):128 * (k0 + kb + 1)] @ Bm[128 * bj:128 * bj + 128, cb:cb + 128].T
            Cm[:, 128 * bj:128 * bj + 128] = acc
    return Cd


# ======================================================================================================================================
# the predictive covariance
# ======================================================================================================================================
PredDesc = collections.namedtuple("PredDesc", "m_pad nkb S family prior noise")
PRED_SIGMA_F, PRED_SN, PRED_ELL, PRED_D, PRED_DP = 1.7, 0.3, 1.3, 5, 8
TOL_PRIOR = 1e-13                                  # tests/test_hip_covariance_inputs.py: the unit covariance's tolerance


def pred_cases():
    """every (m_pad, nkb) with every S <= nkb of {1, 2, 3, 5} and Kss given, the two families alternating and both at every S of nkb = 5;
    one case per covariance function with Kss = NULL"""
    out = []
    for m_pad in (128, 256):
        out.append(PredDesc(m_pad, 1, 1, "normal" if m_pad == 128 else "cancel", "kss", 1))
        for S in (1, 2, 3, 5):
            out.append(PredDesc(m_pad, 5, S, "cancel" if m_pad == 128 else "normal", "kss", S % 2))
    out += [PredDesc(128, 5, 3, "normal", "kss", 0), PredDesc(256, 5, 3, "cancel", "kss", 1), PredDesc(256, 5, 1, "cancel", "kss", 0)]
    out += [PredDesc(256, 5, 3, "normal", "rbf", 1), PredDesc(128, 5, 1, "normal", "matern52", 0)]
    return out


def pred_id(c):
    return "mpad%d-nkb%d-S%d-%s-%s-noise%d" % c


PredLayout = collections.namedtuple("PredLayout", "c P ldz ldk z_elems kss_elems xs_elems part_used part_elems c_elems")


def pred_layout(c):
    cb = c.m_pad // 128
    P = cb * (cb + 1) // 2
    ldz, ldk = 128 * c.nkb + 2, c.m_pad + 2
    used = c.S * P * 128 * 128 if c.S > 1 else 0
    return PredLayout(cb, P, ldz, ldk, c.m_pad * ldz + 8, c.m_pad * ldk + 8, c.m_pad * PRED_DP, used, used + 64, c.m_pad * c.m_pad)


def pred_pairs(c):
    """tile pair p -> (bi, bj): row by row over the lower tile space"""
    return [(bi, bj) for bi in range(c.m_pad // 128) for bj in range(bi + 1)]


def pred_slices(c, mut=None):
    """[kb0, kb1) of every slice.  mut = "slice_boundary": slice 0 runs one block further (needs S > 1)"""
    sl = [(s * c.nkb // c.S, (s + 1) * c.nkb // c.S) for s in range(c.S)]
    if mut == "slice_boundary":
        sl[0] = (sl[0][0], sl[0][1] + 1)
    return sl


@functools.lru_cache(maxsize=None)
def pred_operands(c):
    """Z [m_pad][ldz] (normal: standard normal; cancel: even rows on one pattern, odd rows on an exactly orthogonal one, plus 1e-6 noise: the
    entries between an even and an odd row are 1e-6 of their summed magnitudes), Kss [m_pad][ldk] (not symmetric: the kernel takes its
    symmetric part) or NaN-free Xs [m_pad][dp], zero beyond d.  NaN in the row padding and behind the last row."""
    L = pred_layout(c)
    rng = np.random.default_rng([20266200, c.m_pad, c.nkb, c.family == "cancel", c.prior != "kss"])
    K = 128 * c.nkb
    Z, Kss = np.full(L.z_elems, np.nan), np.full(L.kss_elems, np.nan)
    Zm = Z[:c.m_pad * L.ldz].reshape(c.m_pad, L.ldz)
    Zm[:, :K] = rng.standard_normal((c.m_pad, K))
    if c.family == "cancel":
        p, q = _patterns(rng, K)
        pat = np.where((np.arange(c.m_pad) % 2 == 0)[:, None], p[None, :], q[None, :])
        Zm[:, :K] = pat * rng.uniform(0.5, 2.0, c.m_pad)[:, None] + 1e-6 * Zm[:, :K]
    Kss[:c.m_pad * L.ldk].reshape(c.m_pad, L.ldk)[:, :c.m_pad] = rng.standard_normal((c.m_pad, c.m_pad))
    Xs = np.zeros((c.m_pad, PRED_DP))
    Xs[:, :PRED_D] = rng.standard_normal((c.m_pad, PRED_D))
    ops = dict(Z=Z, Kss=Kss, Xs=Xs.reshape(-1))
    for v in ops.values():
        v.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=None)
def _pred_partial_reference(m_pad, nkb, S, family, given):
    c = PredDesc(m_pad, nkb, S, family, "kss" if given else "rbf", 0)
    L, ops = pred_layout(c), pred_operands(c)
    Zm = ops["Z"][:m_pad * L.ldz].reshape(m_pad, L.ldz)
    ref, bound = np.zeros((S, L.P, 128, 128), dtype=LD), np.zeros((S, L.P, 128, 128), dtype=LD)
    for s, (kb0, kb1) in enumerate(pred_slices(c)):
        for p, (bi, bj) in enumerate(pred_pairs(c)):
            A, B = Zm[128 * bi:128 * bi + 128, 128 * kb0:128 * kb1], Zm[128 * bj:128 * bj + 128, 128 * kb0:128 * kb1]
            ref[s, p] = H.hp_matmul(A, B.T)
            bound[s, p] = (128 * (kb1 - kb0) + 2) * LD(U_RND) * H.hp_matmul(np.abs(A), np.abs(B).T)
    return ref, bound


def pred_partial_reference(c):
    """(ref, bound) [S][P][128][128] long double of the slices' products"""
    return _pred_partial_reference(c.m_pad, c.nkb, c.S, c.family, c.prior == "kss")


def pred_partials_of(c, part, C):
    """[S][P][128][128] view / copy of the partial products as one launch of predcov_partial_kernel left them (S = 1: in C's lower tiles)"""
    L = pred_layout(c)
    if c.S > 1:
        return part[:L.part_used].reshape(c.S, L.P, 128, 128)
    Cm = C.reshape(c.m_pad, c.m_pad)
    return np.stack([Cm[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] for bi, bj in pred_pairs(c)])[None]


def pred_judge_partial(c, part, C):
    """after the partial launch alone: (largest error / bound, sentinels lost): the workspace beyond S P 128^2 and all of C (S > 1); all of
    part and the strictly upper tiles of C (S = 1)"""
    L = pred_layout(c)
    ref, bound = pred_partial_reference(c)
    worst = _ratio(np.abs(pred_partials_of(c, part, C).astype(LD) - ref), bound)
    keep_c = np.ones((c.m_pad, c.m_pad), bool)
    if c.S == 1:
        for bi, bj in pred_pairs(c):
            keep_c[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] = False
    moved = int(np.count_nonzero(~(part.view(np.uint64)[L.part_used:] == SENT_BITS))) + int(np.count_nonzero(~(C.view(np.uint64)[keep_c.reshape(-1)] == SENT_BITS)))
    return worst, moved


def pred_prior(c):
    """(prior [m_pad][m_pad] long double, its magnitude, absolute slack): Kss's symmetric part (slack 0), or the unit covariance of Xs"""
    L, ops = pred_layout(c), pred_operands(c)
    if c.prior == "kss":
        Km = ops["Kss"][:c.m_pad * L.ldk].reshape(c.m_pad, L.ldk)[:, :c.m_pad].astype(LD)
        return (Km + Km.T) / 2, (np.abs(Km) + np.abs(Km.T)) / 2, LD(0)
    X = ops["Xs"].reshape(c.m_pad, PRED_DP).astype(LD)
    sq = np.zeros((c.m_pad, c.m_pad), dtype=LD)
    for k in range(PRED_D):
        df = X[:, k][:, None] - X[:, k][None, :]
        sq += df * df
    ell = LD(PRED_ELL)
    if c.prior == "rbf":
        k = np.exp(-sq / (2 * ell * ell))
    else:
        s = np.sqrt(5 * sq) / ell
        k = (1 + s + s * s / 3) * np.exp(-s)
    return k, k, LD(TOL_PRIOR)


def pred_judge_finish(c, partials, C):
    """(largest error / bound of every entry of C against the long-double finish step on the device's ``partials``, bitwise symmetric?)"""
    prior, pmag, slack = pred_prior(c)
    sums, mags = np.zeros((c.m_pad, c.m_pad), dtype=LD), np.zeros((c.m_pad, c.m_pad), dtype=LD)
    pl = partials.astype(LD)
    for p, (bi, bj) in enumerate(pred_pairs(c)):
        t, ta = pl[:, p].sum(axis=0), np.abs(pl[:, p]).sum(axis=0)
        sums[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128], mags[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] = t, ta
        if bi != bj:
            sums[128 * bj:128 * bj + 128, 128 * bi:128 * bi + 128], mags[128 * bj:128 * bj + 128, 128 * bi:128 * bi + 128] = t.T, ta.T
    low = np.tril(np.ones((c.m_pad, c.m_pad), bool))               # diagonal tiles are computed whole: the finish step reads their lower part
    sums, mags = np.where(low, sums, sums.T), np.where(low, mags, mags.T)
    noise = LD(PRED_SN) * np.eye(c.m_pad, dtype=LD) * c.noise
    sf = LD(PRED_SIGMA_F)
    ref = sf * (prior + noise - sums)
    bound = sf * ((c.S + 4) * LD(U_RND) * (pmag + noise + mags) + slack)
    Cm = C.reshape(c.m_pad, c.m_pad)
    return _ratio(np.abs(Cm.astype(LD) - ref), bound), same_bits(Cm, Cm.T)


def pred_total_bound(c):
    """[m_pad][m_pad]: how far C may lie from the exact sigma_f (prior + noise - Z Z^T): the slices' bounds summed, plus the finish step's"""
    ref, bound = pred_partial_reference(c)
    prior, pmag, slack = pred_prior(c)
    tot, mags = np.zeros((c.m_pad, c.m_pad), dtype=LD), np.zeros((c.m_pad, c.m_pad), dtype=LD)
    for p, (bi, bj) in enumerate(pred_pairs(c)):
        b, a = bound[:, p].sum(axis=0), np.abs(ref[:, p]).sum(axis=0) + bound[:, p].sum(axis=0)
        tot[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128], mags[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] = b, a
        tot[128 * bj:128 * bj + 128, 128 * bi:128 * bi + 128], mags[128 * bj:128 * bj + 128, 128 * bi:128 * bi + 128] = b.T, a.T
    noise = LD(PRED_SN) * np.eye(c.m_pad, dtype=LD) * c.noise
    return LD(PRED_SIGMA_F) * (tot + (c.S + 4) * LD(U_RND) * (pmag + noise + mags) + slack)


def pred_emulate(c, mut=None, finish=True):
    """(part, C) as the entry returns them, in fp64: the slices' products K block by K block, then the finish step -- the partials added
    in slice order, the prior, the noise, sigma_f, the lower triangle mirrored in 32 x 32 sub-tiles.  mut = "slice_boundary": pred_slices';
    "mirror": the mirrored sub-tile is written as it stands, not transposed."""
    L, ops = pred_layout(c), pred_operands(c)
    Zm = ops["Z"][:c.m_pad * L.ldz].reshape(c.m_pad, L.ldz)
    part, C = sentinels(L.part_elems), sentinels(L.c_elems)
    Cm = C.reshape(c.m_pad, c.m_pad)
    prods = np.zeros((c.S, L.P, 128, 128))
    for s, (kb0, kb1) in enumerate(pred_slices(c, mut)):
        for p, (bi, bj) in enumerate(pred_pairs(c)):
            for kb in range(kb0, kb1):
                prods[s, p] += Zm[128 * bi:128 * bi + 128, 128 * kb:128 * kb + 128] @ Zm[128 * bj:128 * bj + 128, 128 * kb:128 * kb + 128].T
    if c.S > 1:
        part[:L.part_used] = prods.reshape(-1)
    else:
        for p, (bi, bj) in enumerate(pred_pairs(c)):
            Cm[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] = prods[0, p]
    if not finish:
        return part, C
    if c.prior == "kss":
        Km = ops["Kss"][:c.m_pad * L.ldk].reshape(c.m_pad, L.ldk)[:, :c.m_pad]
        prior = 0.5 * (Km + Km.T)
    else:
        prior = pred_prior(c)[0].astype(np.float64)
    full = np.zeros((c.m_pad, c.m_pad))
    for p, (bi, bj) in enumerate(pred_pairs(c)):
        acc = np.zeros((128, 128))
        for s in range(c.S):
            acc = acc + prods[s, p]
        full[128 * bi:128 * bi + 128, 128 * bj:128 * bj + 128] = acc
    low = PRED_SIGMA_F * (prior + (PRED_SN * c.noise) * np.eye(c.m_pad) - full)
    out = np.where(np.tril(np.ones((c.m_pad, c.m_pad), bool)), low, low.T)
    if mut == "mirror":
        for I in range(c.m_pad // 32):
            for J in range(I):
                out[32 * J:32 * J + 32, 32 * I:32 * I + 32] = low[32 * I:32 * I + 32, 32 * J:32 * J + 32]
    Cm[:] = out
    return part, C
