"""The tile kernel's operand DMA addresses its slices as scalar base + 32-bit lane offset (csrc/syrk128.hpp, SY_ISSUE): the bases step through
K in scalar registers, in the update kernel and in the strip kernel alike.  The single-launch tests of test_hip_tile_primitives.py pin every
form of the tile bit by bit; what they cannot show is a wrong wait or a wrong base under load (the strip solve's stale rows of round 5 showed
in large lockstep groups only), so here one large group is factored with the updates and the strips of all members in flight together."""
import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

N, D, B = 2048, 8, 32
ELL = 2.5


@pytest.fixture(scope="module")
def S():
    import seaiceextentforecasting_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def group():
    Xb = np.zeros((B, N, D)); yb = np.zeros((B, N)); Xsb = np.zeros((B, 1, D))
    for b in range(B):
        Xb[b], yb[b], Xsb[b] = O.synthetic_problem(N, D, 5100 + b, m=1)
    return Xb, yb, Xsb, np.logspace(-2, -1, B)


def test_lockstep_group_of_32_equals_every_member_alone_twice(S, group):
    """One lockstep group of 32 members at n = 2048 (16 block columns, two outer panels: trailing updates and strip solves of 32 members per
    launch).  Every member's info and outputs are byte-equal to the same member fitted alone, and a second run gives the same bytes.
    Which tile kernel an update gets depends on the tiles per launch (a lone n = 2048 fit is below `small_tile_threshold`
    and takes the generic 64 x 64 kernel, another k order), so both sides run with the threshold at 0 and strip panels: the same tile
    kernels alone and under load.  With the default threshold the group differs from the lone fits in the last bits, on the parent
    commit and on this one alike (worst relative difference mean 6.1e-13, nlml 7.5e-15, sigma_f 8.9e-15, var 8.9e-15)."""
    Xb, yb, Xsb, sn = group
    runs = []
    for _ in range(2):
        with S.GPR(kernel="rbf", outer_blocks=8, panel_mode="strips") as gp:
            gp.set_option("small_tile_threshold", 0)
            runs.append(gp.fit_batch(Xb, yb, Xsb, np.full(B, ELL), sn, concurrency=1, group=B))
    for key in ("info", "nlml", "sigma_f", "mean", "var"):
        assert np.array_equal(np.asarray(runs[0][key]), np.asarray(runs[1][key])), key
    r = runs[0]
    assert np.all(np.asarray(r["info"]) == 0)
    worst = {}
    for b in range(B):
        with S.GPR(kernel="rbf", outer_blocks=8, panel_mode="strips") as gp:
            gp.set_option("small_tile_threshold", 0)
            gp.fit(Xb[b], yb[b], ELL, sn[b], Xs=Xsb[b])
            mu, var = gp.predict(Xsb[b])
            alone = {"nlml": gp.nlml_, "sigma_f": gp.sigma_f_, "mean": mu, "var": var}
        for key, v in alone.items():
            a, c = np.ravel(np.asarray(r[key][b], dtype=np.float64)), np.ravel(np.asarray(v, dtype=np.float64))
            worst[key] = max(worst.get(key, 0.0), float(np.max(np.abs(a - c) / np.maximum(np.abs(c), 1e-300))))
    print("lockstep group vs alone, worst relative difference per output:", worst)
    assert all(w == 0.0 for w in worst.values()), worst
