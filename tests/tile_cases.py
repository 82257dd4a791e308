"""Descriptors of single launches of the MFMA tile primitives, and what such a launch must do to memory, in plain NumPy: which tiles
a descriptor owns and over which k span (the rules of ``gemm_tile_coords`` / ``gemm_tile_body`` / ``syrk128_kernel``, restated here
and checked against the C++ by tests/test_tile_walk_host.py), buffers with sentinels and NaNs around everything the launch may
touch, the long-double value of every owned entry and its forward bound.  Shared by tests/test_hip_tile_primitives.py (GPU) and the
host tier; nothing here needs a GPU.

Layout of a case (elements; every stride a multiple of 16 bytes):
    A   [rows_a][lda = K + pad]   per member, members ``GAP`` elements apart (``shared_a``: the batch axis re-uses one A, sA = 0)
    B   [cols][ldb = K + pad]     or, B transposed, [K][ldb = cols + pad];  ``alias``: B IS A (one buffer, the launch sees one pointer)
    C   [rows][ldc = cols + pad]
batch member y and second-axis member z sit at y * s? + z * z?.  Window, ``lower``, ``ktri``, ``zshift``, ride row: GemmArgsT.
"""
import collections

import numpy as np

import hp_reference as H

LD = H.LD
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
NPT = {"f64": np.float64, "f32": np.float32}
BITS = {"f64": np.uint64, "f32": np.uint32}
SLICE = {"f64": 16, "f32": 32}                     # K-slice: 128 bytes per row
NE = {"f64": 2, "f32": 4}                          # elements per 16 bytes
SENTINEL = {"f64": np.uint64(0x7FF8DEADBEEF0BAD), "f32": np.uint32(0x7FC0BEEF)}     # quiet NaNs with a payload nothing computes
GAP = 8

Cfg = collections.namedtuple("Cfg", "id tm tn mode bt kind")
# include/sigp_debug.h, sigp_debug_run_gemm
CFGS = {
    "32x128_set": Cfg(0, 32, 128, "set", False, "gemm"), "32x128_set_bt": Cfg(1, 32, 128, "set", True, "gemm"),
    "32x128_setneg_bt": Cfg(2, 32, 128, "setneg", True, "gemm"), "64x64_set": Cfg(3, 64, 64, "set", False, "gemm"),
    "64x64_sub": Cfg(4, 64, 64, "sub", False, "gemm"), "64x64_sub_bt": Cfg(5, 64, 64, "sub", True, "gemm"),
    "128x128_sub": Cfg(6, 128, 128, "sub", False, "gemm"), "128x128_setneg_bt": Cfg(7, 128, 128, "setneg", True, "gemm"),
    "32x32_sub": Cfg(8, 32, 32, "sub", False, "gemm"), "syrk128_sub": Cfg(9, 128, 128, "sub", False, "syrk"),
    "syrk128_set": Cfg(10, 128, 128, "set", False, "syrk"), "auto": Cfg(11, 128, 128, "sub", False, "auto"),
}

_DEFAULTS = collections.OrderedDict(
    dtype="f64", cfg="64x64_sub", K=48, win=(0, 1, 0, 1), lower=0, ktri=0, batch=1, zcount=1, zshift=0, ride=(0, 0), pad=0, shared_a=False,
    alias=False, family="normal", diag_tiles=1, opts=())
Desc = collections.namedtuple("Desc", list(_DEFAULTS))


def desc(**kw):
    d = dict(_DEFAULTS)
    d.update(kw)
    return Desc(**d)


def case_id(d):
    parts = [d.cfg, d.dtype, "K%d" % d.K, "w%d.%d.%d.%d" % d.win]
    for k, v in d._asdict().items():
        if k not in ("cfg", "dtype", "K", "win") and v != _DEFAULTS[k]:
            parts.append("%s=%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v))
    return "-".join(parts).replace(" ", "").replace("'", "").replace("(", "").replace(")", "").replace(",", ".")


Layout = collections.namedtuple("Layout", "tm tn nby nbz rows cols rows_a rows_b cols_b lda ldb ldc sA sB sC zA zB zC a_elems b_elems c_elems")


def layout(d):
    c = CFGS[d.cfg]
    r0, r1, c0, c1 = d.win
    nby, nbz = max(1, d.batch), max(1, d.zcount)
    rows, cols = max(r1, 1) * c.tm, max(c1, 1) * c.tn
    rows_a = max(rows, cols) if d.alias else rows
    lda = d.K + d.pad
    blk = rows_a * lda
    sA = 0 if d.shared_a else blk + GAP
    zA = (nby - 1) * sA + blk + GAP
    a_elems = (nbz - 1) * zA + (nby - 1) * sA + blk + GAP
    if d.alias:
        assert c.tm == c.tn and not c.bt
        rows_b, cols_b, ldb, sB, zB, b_elems = rows_a, d.K, lda, sA, zA, 0
    else:
        rows_b, cols_b = (d.K, cols) if c.bt else (cols, d.K)
        ldb = cols_b + d.pad
        sB = rows_b * ldb + GAP
        zB = (nby - 1) * sB + rows_b * ldb + GAP
        b_elems = (nbz - 1) * zB + (nby - 1) * sB + rows_b * ldb + GAP
    ldc = cols + d.pad
    sC = rows * ldc + GAP
    zC = (nby - 1) * sC + rows * ldc + GAP
    c_elems = (nbz - 1) * zC + (nby - 1) * sC + rows * ldc + GAP
    return Layout(c.tm, c.tn, nby, nbz, rows, cols, rows_a, rows_b, cols_b, lda, ldb, ldc, sA, sB, sC, zA, zB, zC, a_elems, b_elems, c_elems)


def view(buf, base, rows, ld):
    """[rows][ld] view of a flat buffer from element ``base``"""
    return buf[base:base + rows * ld].reshape(rows, ld)


def owned_tiles(d, y=0):
    """(bi, bj) of the tiles batch member y owns: columns [c0, c1), rows [max(r0, lower ? bj + zshift y : r0), r1)"""
    r0, r1, c0, c1 = d.win
    out = []
    for bj in range(c0, c1):
        lo = max(r0, bj + d.zshift * y) if d.lower else r0
        out.extend((bi, bj) for bi in range(lo, r1))
    return out


def tile_k(d, bi, bj):
    """[k0, k1) of a tile: ktri = 1 starts at the row block's first column, ktri = 2 stops after the column block's last row"""
    c = CFGS[d.cfg]
    k0 = bi * c.tm if d.ktri == 1 else 0
    k1 = min(d.K, (bj + 1) * c.tn) if d.ktri == 2 else d.K
    return k0, k1


def diag_skip_launch(d):
    """does launch_syrk128_t pick the diagonal-skip instantiation (DG diagonal tiles, RD ride tiles) for this descriptor?"""
    return bool(CFGS[d.cfg].kind == "syrk" and CFGS[d.cfg].mode == "sub" and d.diag_tiles and d.lower and d.alias and d.win[0] <= d.win[2])


def members(d, L):
    return [(y, z) for z in range(L.nbz) for y in range(L.nby)]


def masks(d):
    """dict(check, unspec: bool [c_elems]; readA [a_elems], readB [b_elems or a_elems]).  check = entries whose value the descriptor
    defines; unspec = the strictly upper part of diagonal tiles where the kernel may or may not write (the DG form, and `auto`, whose
    64- and 32-unit walks own fewer sub-tiles above the diagonal than the 128-unit one); everything else must keep its bits -- that
    includes rows >= 16 of a ride-row tile, which the RD form neither reads nor writes and every other form updates with exact zeros."""
    c, L = CFGS[d.cfg], layout(d)
    check, unspec = np.zeros(L.c_elems, bool), np.zeros(L.c_elems, bool)
    readA = np.zeros(L.a_elems, bool)
    readB = readA if d.alias else np.zeros(L.b_elems, bool)
    upper = np.triu(np.ones((c.tm, c.tn), bool), 1)
    loose_diag = d.lower and (diag_skip_launch(d) or c.kind == "auto")
    for y, z in members(d, L):
        Cm, Um = view(check, y * L.sC + z * L.zC, L.rows, L.ldc), view(unspec, y * L.sC + z * L.zC, L.rows, L.ldc)
        Am = view(readA, y * L.sA + z * L.zA, L.rows_a, L.lda)
        Bm = view(readB, y * L.sB + z * L.zB, L.rows_b, L.ldb)
        for bi, bj in owned_tiles(d, y):
            k0, k1 = tile_k(d, bi, bj)
            rs, cs = slice(bi * c.tm, (bi + 1) * c.tm), slice(bj * c.tn, (bj + 1) * c.tn)
            t = np.ones((c.tm, c.tn), bool)
            if loose_diag and bi == bj:
                t &= ~upper
                Um[rs, cs] |= upper
            if d.ride[0] > 0 and bi == d.ride[0] - 1:
                t[16:] = False
            Cm[rs, cs] |= t
            Am[rs, k0:k1] = True
            if c.bt:
                Bm[k0:k1, cs] = True
            else:
                Bm[cs, k0:k1] = True
    unspec &= ~check
    return dict(check=check, unspec=unspec, readA=readA, readB=readB)


def ride_rest(d):
    """bool [c_elems]: rows 16 .. of the ride-row tiles -- what the RD form neither reads nor writes"""
    c, L = CFGS[d.cfg], layout(d)
    rest = np.zeros(L.c_elems, bool)
    for y, z in members(d, L):
        Rm = view(rest, y * L.sC + z * L.zC, L.rows, L.ldc)
        for bi, bj in owned_tiles(d, y):
            if d.ride[0] > 0 and bi == d.ride[0] - 1:
                Rm[bi * c.tm + 16:(bi + 1) * c.tm, bj * c.tn:(bj + 1) * c.tn] = True
    return rest


def _cancel_pair(rng, rows, K):
    """(P, Q) [rows][K] with P_i . Q_j = 0 exactly over every aligned pair of columns, in any precision the entries are rounded to:
    P[:, 2m] = P[:, 2m+1], Q[:, 2m] = -Q[:, 2m+1]"""
    v, w = rng.standard_normal(K // 2), rng.standard_normal(K // 2)
    return np.repeat(v, 2)[None, :] * rng.uniform(0.5, 2.0, rows[0])[:, None], \
        (np.repeat(w, 2) * np.tile([1.0, -1.0], K // 2))[None, :] * rng.uniform(0.5, 2.0, rows[1])[:, None]


def operands(d, seed=0):
    """dict(A, B (None when aliased), C: flat arrays of the working type as the launch is given them; C0: the values under the owned
    tiles (SUB) as float64).  ``normal``: standard normal.  ``cancel``: results 1e-6 of the summed magnitudes -- SET forms: rows of A
    and B built on two exactly orthogonal patterns plus 1e-6 noise; SUB forms: C0 = the product to 1e-6 -- and one K-slice (the last;
    the first under ktri = 2) 1e-8 of the others, so that a dropped or doubled slice moves a result by ~1e-2 of its size while the
    bound is ~K u 1e6 of it.  Then NaN in every element of A and B that no owned tile reads (row and member gaps, tiles outside the window,
    the k range a triangular span skips), the sentinel in every element of C outside the owned tiles -- and inside them too for
    the SET forms, which must not read C."""
    c, L, t = CFGS[d.cfg], layout(d), NPT[d.dtype]
    rng = np.random.default_rng([seed, c.id, d.K, L.c_elems])
    m = masks(d)
    A = rng.standard_normal(L.a_elems)
    B = None if d.alias else rng.standard_normal(L.b_elems)
    S = SLICE[d.dtype]
    ks = 0 if d.ktri == 2 else d.K - S
    for y, z in members(d, L):
        if d.shared_a and y > 0:
            continue
        Am = view(A, y * L.sA + z * L.zA, L.rows_a, L.lda)
        if d.family == "cancel":
            if c.mode != "sub" and not d.alias:
                Bm = view(B, y * L.sB + z * L.zB, L.rows_b, L.ldb)
                P, Q = _cancel_pair(rng, (L.rows_a, L.cols), d.K)
                Am[:, :d.K] = P + 1e-6 * Am[:, :d.K]
                if c.bt:
                    Bm[:, :L.cols] = Q.T + 1e-6 * Bm[:, :L.cols]
                else:
                    Bm[:, :d.K] = Q + 1e-6 * Bm[:, :d.K]
            Am[:, ks:ks + S] *= 1e-4 if d.alias else 1e-8
        if d.ride[0] > 0:
            Am[(d.ride[0] - 1) * c.tm + d.ride[1]:d.ride[0] * c.tm] = 0.0           # the ride block's rows not in use are zero rows
    A = A.astype(t)
    B = None if B is None else B.astype(t)
    C0 = rng.standard_normal(L.c_elems)
    if d.family == "cancel" and c.mode == "sub":
        Bsrc = A if d.alias else B
        for y, z in members(d, L):
            Am = view(A, y * L.sA + z * L.zA, L.rows_a, L.lda).astype(np.float64)
            Bm = view(Bsrc, y * L.sB + z * L.zB, L.rows_b, L.ldb).astype(np.float64)
            Cm = view(C0, y * L.sC + z * L.zC, L.rows, L.ldc)
            for bi, bj in owned_tiles(d, y):
                k0, k1 = tile_k(d, bi, bj)
                rs, cs = slice(bi * c.tm, (bi + 1) * c.tm), slice(bj * c.tn, (bj + 1) * c.tn)
                Bt = Bm[k0:k1, cs] if c.bt else Bm[cs, k0:k1].T
                prod = Am[rs, k0:k1] @ Bt
                Cm[rs, cs] = np.where(prod != 0.0, prod * (1.0 + 1e-6 * Cm[rs, cs]), Cm[rs, cs])   # (zero rows of a ride block: no signed zeros in C0)
    C0 = C0.astype(t)
    A[~m["readA"]] = np.nan
    if B is not None:
        B[~m["readB"]] = np.nan
    C = np.full(L.c_elems, SENTINEL[d.dtype], dtype=BITS[d.dtype]).view(t)
    if c.mode == "sub":
        own = np.zeros(L.c_elems, bool)
        for y, z in members(d, L):
            Om = view(own, y * L.sC + z * L.zC, L.rows, L.ldc)
            for bi, bj in owned_tiles(d, y):
                Om[bi * c.tm:(bi + 1) * c.tm, bj * c.tn:(bj + 1) * c.tn] = True
        C[own] = C0[own]
    return dict(A=A, B=B, C=C, C0=C0.astype(np.float64))


def reference(d, ops):
    """(ref, bound): long-double value of every checked entry (NaN elsewhere) and (K_eff + 2) u (|A| |B|^T + |C0|), K_eff the tile's
    k span, u the unit roundoff of the working type; operands widened from the working type, C0 counted for the SUB forms only (the
    others do not read C)."""
    c, L = CFGS[d.cfg], layout(d)
    ref, bound = np.full(L.c_elems, np.nan, dtype=LD), np.full(L.c_elems, np.nan, dtype=LD)
    Bsrc = ops["A"] if d.alias else ops["B"]
    u = LD(UNIT[d.dtype])
    for y, z in members(d, L):
        Am = view(ops["A"], y * L.sA + z * L.zA, L.rows_a, L.lda)
        Bm = view(Bsrc, y * L.sB + z * L.zB, L.rows_b, L.ldb)
        C0 = view(ops["C0"], y * L.sC + z * L.zC, L.rows, L.ldc)
        Rm, Bd = view(ref, y * L.sC + z * L.zC, L.rows, L.ldc), view(bound, y * L.sC + z * L.zC, L.rows, L.ldc)
        for bi, bj in owned_tiles(d, y):
            k0, k1 = tile_k(d, bi, bj)
            rs, cs = slice(bi * c.tm, (bi + 1) * c.tm), slice(bj * c.tn, (bj + 1) * c.tn)
            At = Am[rs, k0:k1]
            Bt = Bm[k0:k1, cs] if c.bt else Bm[cs, k0:k1].T
            P = H.hp_matmul(At, Bt)
            mag = H.hp_matmul(np.abs(At), np.abs(Bt))
            if c.mode == "sub":
                Rm[rs, cs] = C0[rs, cs].astype(LD) - P
                mag = mag + np.abs(C0[rs, cs])
            else:
                Rm[rs, cs] = P if c.mode == "set" else -P
            Bd[rs, cs] = (k1 - k0 + 2) * u * mag
    return ref, bound


def judge(d, ops, dev, ref, bound, m=None):
    """(largest |dev - ref| / bound over the checked entries, number of entries outside check / unspec whose bits changed)"""
    m = m or masks(d)
    ck = m["check"]
    e = np.abs(dev[ck].astype(LD) - ref[ck])
    b = bound[ck]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(e == 0, LD(0), e / b)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)            # a NaN result, or an error where the bound is zero
    keep = ~(ck | m["unspec"])
    bt = BITS[d.dtype]
    moved = int(np.count_nonzero(dev.view(bt)[keep] != ops["C"].view(bt)[keep]))
    return float(ratio.max()) if ratio.size else 0.0, moved


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def gemm_cases():
    """Every descriptor the GPU file launches through sigp_debug_run_gemm (and the host tier walks): the smallest shapes at which each
    mechanism exists."""
    out = []
    add = lambda **kw: out.append(desc(**kw))   # noqa: E731
    for dt in ("f64", "f32"):
        S, P = SLICE[dt], NE[dt]
        # every instantiation: one slice, 48 / 96, 128, and a padded leading dimension; both operand families
        for cfg in CFGS:
            if cfg == "auto":
                continue
            al = CFGS[cfg].kind == "syrk" and CFGS[cfg].mode == "sub"
            add(dtype=dt, cfg=cfg, K=S)
            add(dtype=dt, cfg=cfg, K=3 * S, pad=P, family="cancel")
            add(dtype=dt, cfg=cfg, K=128, win=(1, 3, 0, 2), pad=P)
            if al:
                add(dtype=dt, cfg=cfg, K=128, win=(0, 3, 0, 3), lower=1, alias=True, family="cancel")
        # K = 2048 on the update kernels, one tile (the reference costs the time)
        add(dtype=dt, cfg="syrk128_sub", K=2048, family="cancel")
        add(dtype=dt, cfg="128x128_sub", K=2048)
        add(dtype=dt, cfg="64x64_sub", K=2048, family="cancel")
    # windows, lower or not (fp64; K = 48)
    for cfg in ("64x64_sub", "32x32_sub", "syrk128_sub", "32x128_set"):
        for win in ((1, 3, 0, 2), (2, 5, 2, 5)):
            for lower in (0, 1):
                add(cfg=cfg, win=win, lower=lower, pad=2)
    add(cfg="64x64_sub", win=(2, 2, 0, 2))                                            # empty windows: nothing is launched, nothing moves
    add(cfg="syrk128_sub", win=(0, 2, 1, 1), lower=1)
    add(cfg="64x64_sub", win=(2, 4, 0, 3), lower=1)                                   # r0 > c0, lower
    add(cfg="syrk128_sub", win=(1, 3, 0, 3), lower=1, alias=True)                     # r0 > c0: launch_syrk128_t must not take the DG form
    add(cfg="syrk128_sub", win=(2, 5, 2, 5), lower=1, alias=True, pad=2)              # DG tiles off the origin
    add(cfg="syrk128_sub", win=(0, 3, 0, 3), lower=1, alias=True, diag_tiles=0)
    add(dtype="f32", cfg="syrk128_sub", win=(0, 2, 0, 2), K=64, lower=1, alias=True, pad=4)
    # members
    for cfg in ("64x64_sub", "syrk128_sub", "syrk128_set", "32x128_setneg_bt"):
        add(cfg=cfg, win=(0, 2, 0, 1), batch=3)
        add(cfg=cfg, win=(0, 2, 0, 1), batch=3, shared_a=True, pad=2)
        add(cfg=cfg, win=(0, 1, 0, 2), batch=2, zcount=2)
    for zs in (0, 1):
        add(cfg="64x64_sub", win=(0, 3, 0, 3), lower=1, batch=2, zcount=2, zshift=zs)
        add(cfg="syrk128_sub", win=(0, 3, 0, 3), lower=1, batch=2, zcount=2, zshift=zs, alias=True)
        add(dtype="f32", cfg="syrk128_sub", K=64, win=(0, 3, 0, 2), lower=1, batch=2, zcount=2, zshift=zs)
    # triangular K spans: operands carry NaN where the span must not reach
    for dt in ("f64", "f32"):
        add(dtype=dt, cfg="syrk128_set", K=384, win=(0, 3, 0, 2), ktri=1)                # trtri_levels' first product
        add(dtype=dt, cfg="syrk128_sub", K=384, win=(0, 3, 0, 3), ktri=1, lower=1, alias=True)
        add(dtype=dt, cfg="syrk128_sub", K=384, win=(0, 3, 0, 3), ktri=1, lower=1, alias=True, diag_tiles=0, family="cancel")
        add(dtype=dt, cfg="64x64_sub", K=192, win=(1, 3, 0, 2), ktri=1)
        add(dtype=dt, cfg="64x64_sub", K=192, win=(0, 3, 0, 3), ktri=1, lower=1)
        add(dtype=dt, cfg="64x64_sub_bt", K=192, win=(0, 3, 0, 2), ktri=1)
        add(dtype=dt, cfg="128x128_setneg_bt", K=384, win=(0, 2, 0, 3), ktri=2, batch=2)  # trtri_levels' second product
        add(dtype=dt, cfg="64x64_sub_bt", K=192, win=(0, 2, 1, 3), ktri=2, pad=NE[dt], family="cancel")
        add(dtype=dt, cfg="32x128_set_bt", K=256, win=(1, 3, 0, 2), ktri=2)
    # the ride row (RD form): block row 2 of a 3 x 3 symmetric update with 1, 3 and 16 rows in use
    for dt in ("f64", "f32"):
        for rows in (1, 3, 16):
            add(dtype=dt, cfg="syrk128_sub", K=4 * SLICE[dt], win=(0, 3, 0, 3), lower=1, alias=True, ride=(3, rows))
    add(cfg="syrk128_sub", K=128, win=(0, 3, 0, 2), lower=1, alias=True, ride=(3, 3), batch=2, family="cancel")
    return out


def auto_cases():
    """gemm_sub_auto's branches: a five-tile window either side of small_tile_threshold (syrk128_kernel | the small-tile kernels) and of
    tiny_tile_threshold (32x32 | 64x64 tiles, short K only: K = 256 takes them, K = 384 does not).  opts = handle options."""
    out = []
    for dt in ("f64", "f32"):
        for win, lower, alias in (((0, 1, 0, 5), 0, False), ((0, 3, 0, 2), 1, True)):     # 5 tiles each
            base = dict(dtype=dt, cfg="auto", win=win, lower=lower, alias=alias, K=256)
            out.append(desc(opts=(("small_tile_threshold", 5), ("tiny_tile_threshold", 0)), **base))        # nt >= small: syrk128
            out.append(desc(opts=(("small_tile_threshold", 6), ("tiny_tile_threshold", 19)), **base))       # below; 4 nt > tiny: 64x64
            out.append(desc(opts=(("small_tile_threshold", 6), ("tiny_tile_threshold", 20)), **base))       # 4 nt <= tiny: 32x32
            base["K"] = 384
            out.append(desc(opts=(("small_tile_threshold", 6), ("tiny_tile_threshold", 20)), **base))       # long K: 64x64 again
    out.append(desc(cfg="auto", win=(0, 3, 0, 3), lower=1, alias=True, K=128, ride=(3, 2), opts=(("small_tile_threshold", 1),)))
    out.append(desc(cfg="auto", win=(0, 3, 0, 3), lower=1, alias=True, K=128, ride=(3, 2), opts=(("small_tile_threshold", 100), ("tiny_tile_threshold", 0))))
    return out


def refused_cases():
    """descriptors sigp_debug_run_gemm must answer with SIGP_BAD_ARG: (what, Desc, overrides of the call's arguments)"""
    return [
        ("K not a multiple of the slice", desc(K=40), {}),
        ("fp32 K = 16", desc(dtype="f32", K=16), {}),
        ("fp32 leading dimension + 2: 8 bytes", desc(dtype="f32", K=32), {"lda": 34}),
        ("A one element short", desc(), {"a_elems": -GAP - 1}),
        ("C one element short", desc(), {"c_elems": -GAP - 1}),
        ("B one element short", desc(), {"b_elems": -GAP - 1}),
        ("window past the buffers", desc(win=(0, 1, 0, 1)), {"r1": 2}),
        ("ktri = 1 with an empty span", desc(cfg="syrk128_set", K=128, win=(0, 2, 0, 1), ktri=1), {}),
        ("ktri = 2 on syrk128", desc(cfg="syrk128_set", K=128, ktri=2), {}),
        ("ktri with auto", desc(cfg="auto", K=128, ktri=1), {}),
        ("zshift without lower", desc(win=(0, 2, 0, 2), batch=2, zshift=1), {}),
        ("zshift with ktri = 1", desc(K=192, win=(0, 3, 0, 3), lower=1, ktri=1, batch=2, zshift=1), {}),
        ("negative zshift", desc(win=(0, 2, 0, 2), lower=1, batch=2), {"zshift": -1}),
        ("17 ride rows", desc(cfg="syrk128_sub", win=(0, 2, 0, 2), lower=1, alias=True, ride=(2, 16)), {"ride_rows": 17}),
        ("members on one C", desc(batch=2), {"sC": 0}),
        ("unknown cfg", desc(), {"cfg": 12}),
    ]
