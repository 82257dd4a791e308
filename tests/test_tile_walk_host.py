"""Host tier of tests/test_hip_tile_primitives.py.

1. The tile walk.  ``gemm_tile_count`` / ``gemm_grid_size`` / ``gemm_tile_coords`` are plain integer code in csrc/gemm_mfma.hpp; the text of
   the descriptor and of the three functions is compiled into a stand-alone host program (address + undefined-behaviour sanitizers on)
   that walks blockIdx.x over the grid of every descriptor the GPU file launches, for every batch member, and prints the tiles.  Each
   owned tile must come out exactly once, none other, and the grid must be the size the launchers give it -- and the list must be the one
   tests/tile_cases.py derives its footprints and references from.
2. The helpers themselves -- footprint masks, k spans, long-double reference, bound, hp_matmul -- against element-by-element Python loops
   on two-tile cases.
"""
import os
import subprocess

import numpy as np
import pytest

import hp_reference as H
import tile_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "seaiceextentforecasting_amd", "csrc", "gemm_mfma.hpp")

MAIN = r'''
#include <cstdio>
int main() {
  int r0, r1, c0, c1, lower, ktri, zshift, y;
  while (std::scanf("%d %d %d %d %d %d %d %d", &r0, &r1, &c0, &c1, &lower, &ktri, &zshift, &y) == 8) {
    GemmArgsT<double> g{};
    g.r0 = r0; g.r1 = r1; g.c0 = c0; g.c1 = c1; g.lower = lower; g.ktri = ktri; g.zshift = zshift; g.patch = 0;
    blockIdx.y = (unsigned)y;
    const int grid = gemm_grid_size(r0, r1, c0, c1, lower, 0);
    std::printf("%d %d", grid, gemm_tile_count(r0, r1, c0, c1, lower));
    for (int b = 0; b < grid; ++b) { int bi = -1, bj = -1; if (gemm_tile_coords(g, b, bi, bj)) std::printf(" %d:%d", bi, bj); }
    std::printf("\n");
  }
  return 0;
}
'''


def all_descriptors():
    return TC.gemm_cases() + TC.auto_cases()


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    text = open(HDR).read()
    a, b = text.index("template <typename T>\nstruct GemmArgsT {"), text.index("// XCD-chunked walk")
    assert 0 < a < b
    src = tmp_path_factory.mktemp("walk") / "walk.cpp"
    src.write_text("#include <algorithm>\n#define __host__\n#define __device__\nstatic struct { unsigned x, y, z; } blockIdx;\n" + text[a:b] + MAIN)
    exe = src.with_suffix("")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(src)])
    return str(exe)


def test_case_ids_are_unique():
    ids = [TC.case_id(d) for d in all_descriptors()]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)


def test_the_walk_hands_out_every_owned_tile_exactly_once(walker):
    queries = []
    for d in all_descriptors():
        scale = (1, 2, 4) if d.cfg == "auto" else (1,)           # gemm_sub_auto: the same region in 128-, 64- and 32-units
        for s in scale:
            for y in range(max(1, d.batch)):
                queries.append((d, s, y))
    lines = "".join("%d %d %d %d %d %d %d %d\n" % (tuple(s * w for w in d.win) + (d.lower, d.ktri, s * d.zshift, y)) for d, s, y in queries)
    p = subprocess.run([walker], input=lines, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = p.stdout.strip().split("\n")
    assert len(rows) == len(queries)
    for (d, s, y), row in zip(queries, rows):
        f = row.split()
        grid, count = int(f[0]), int(f[1])
        got = [tuple(int(v) for v in t.split(":")) for t in f[2:]]
        ds = d._replace(win=tuple(s * w for w in d.win), zshift=s * d.zshift)
        want = TC.owned_tiles(ds, y)
        assert len(got) == len(set(got)), (TC.case_id(d), s, y, "a tile handed out twice")
        assert sorted(got) == sorted(want), (TC.case_id(d), s, y)
        assert grid == count == len(TC.owned_tiles(ds, 0)), (TC.case_id(d), s, y, "the grid is sized for member 0")


def test_auto_units_cover_the_same_entries_below_the_diagonal():
    """the 64- and 32-unit walks of a lower window own every entry on or below the diagonal of the 128-unit one, and nothing outside it"""
    for win in ((0, 3, 0, 2), (0, 3, 0, 3), (1, 3, 0, 2)):
        n = 128 * 3
        big = np.zeros((n, n), bool)
        for bi, bj in TC.owned_tiles(TC.desc(win=win, lower=1)):
            big[bi * 128:(bi + 1) * 128, bj * 128:(bj + 1) * 128] = True
        for s in (2, 4):
            t = 128 // s
            small = np.zeros((n, n), bool)
            for bi, bj in TC.owned_tiles(TC.desc(win=tuple(s * w for w in win), lower=1)):
                small[bi * t:(bi + 1) * t, bj * t:(bj + 1) * t] = True
            assert not np.any(small & ~big)
            assert np.array_equal(np.tril(small), np.tril(big))


def test_hp_matmul_is_a_loop_of_long_double_dots():
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((70, 33)).astype(np.float32), rng.standard_normal((33, 9))
    got = H.hp_matmul(A, B)
    assert got.dtype == H.LD
    for i in range(70):
        for j in range(9):
            s = H.LD(0)
            for k in range(33):
                s += H.LD(A[i, k]) * H.LD(B[k, j])
            assert abs(got[i, j] - s) <= 40 * np.finfo(H.LD).eps * float(np.abs(A[i]).astype(np.float64) @ np.abs(B[:, j]))


BRUTE = [TC.desc(cfg="32x32_sub", K=48, win=(0, 2, 0, 1), pad=2),
         TC.desc(cfg="32x32_sub", K=64, win=(0, 2, 0, 2), lower=1, ktri=1, batch=2, family="cancel"),
         TC.desc(dtype="f32", cfg="64x64_sub_bt", K=128, win=(0, 1, 0, 2), ktri=2, pad=4),
         TC.desc(cfg="32x128_setneg_bt", K=32, win=(1, 3, 0, 1), zcount=2),
         TC.desc(cfg="64x64_sub", K=32, win=(0, 2, 0, 2), lower=1, batch=2, zshift=1, shared_a=True)]


@pytest.mark.skipif(not H.AVAILABLE, reason="np.longdouble is not an extended type here (eps >= 1e-18)")
@pytest.mark.parametrize("d", BRUTE, ids=TC.case_id)
def test_footprint_and_reference_against_an_element_loop(d):
    c, L = TC.CFGS[d.cfg], TC.layout(d)
    ops, m = TC.operands(d, seed=3), TC.masks(d)
    ref, bound = TC.reference(d, ops)
    r0, r1, c0, c1 = d.win
    A, B, C0 = ops["A"], ops["B"], ops["C0"]
    check = np.zeros(L.c_elems, bool)
    usedA, usedB = np.zeros(L.a_elems, bool), np.zeros(L.b_elems, bool)
    u = TC.UNIT[d.dtype]
    for z in range(L.nbz):
        for y in range(L.nby):
            for i in range(L.rows):
                for j in range(L.cols):
                    bi, bj = i // c.tm, j // c.tn
                    if not (r0 <= bi < r1 and c0 <= bj < c1) or (d.lower and bi < bj + d.zshift * y):
                        continue
                    k0 = bi * c.tm if d.ktri == 1 else 0
                    k1 = min(d.K, (bj + 1) * c.tn) if d.ktri == 2 else d.K
                    e = y * L.sC + z * L.zC + i * L.ldc + j
                    ia = y * L.sA + z * L.zA + i * L.lda + np.arange(k0, k1)
                    ib = y * L.sB + z * L.zB + (np.arange(k0, k1) * L.ldb + j if c.bt else j * L.ldb + np.arange(k0, k1))
                    check[e], usedA[ia], usedB[ib] = True, True, True
                    a, b = A[ia].astype(H.LD), B[ib].astype(H.LD)
                    dot = H.LD(0)
                    for k in range(k1 - k0):
                        dot += a[k] * b[k]
                    want = {"sub": H.LD(C0[e]) - dot, "set": dot, "setneg": -dot}[c.mode]
                    mag = np.sum(np.abs(a) * np.abs(b)) + (abs(H.LD(C0[e])) if c.mode == "sub" else 0)
                    assert abs(ref[e] - want) <= 1e-17 * float(mag) + 1e-300
                    assert abs(bound[e] - (k1 - k0 + 2) * u * mag) <= 1e-12 * float(bound[e])
    assert np.array_equal(check, m["check"]) and not m["unspec"].any()
    assert np.array_equal(usedA, m["readA"]) and np.array_equal(usedB, m["readB"])
    assert np.array_equal(np.isnan(A), ~usedA) and np.array_equal(np.isnan(B), ~usedB)              # NaN exactly where nothing reads
    bits = TC.BITS[d.dtype]
    owned_sub = check if c.mode == "sub" else np.zeros_like(check)
    assert np.all(ops["C"].view(bits)[~owned_sub] == TC.SENTINEL[d.dtype])
    assert np.array_equal(ops["C"][owned_sub].astype(np.float64), C0[owned_sub])
    assert np.all(np.isnan(ref[~check]))
    dev = ops["C"].copy()
    dev[check] = ref[check].astype(TC.NPT[d.dtype])                                                  # a correctly rounded "device"
    ratio, moved = TC.judge(d, ops, dev, ref, bound, m)
    assert ratio <= 1.0 and moved == 0
    bad = dev.copy()
    bad[np.flatnonzero(~check)[0]] = 1.0                                                              # one stray store
    first = np.flatnonzero(check)[0]
    bad[first] += 4 * float(bound[first]) + abs(bad[first]) * 4 * u                                   # one value outside its bound
    ratio, moved = TC.judge(d, ops, bad, ref, bound, m)
    assert ratio > 1.0 and moved == 1
