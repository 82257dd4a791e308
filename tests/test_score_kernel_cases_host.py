"""Host tier of tests/score_kernel_cases.py (no GPU): an fp64 NumPy emulation of each kernel's formula -- the Gram form in the tile's local
coordinates, the expanded square, the slices' sums in the kernels' order -- goes through the judges the GPU tests use.  The unmutated emulation
must pass every case; every mutation must exceed its bound by at least a factor of 10 in every case where it applies.  That second half is
what keeps the bounds from hiding a failure: a bound a wrong kernel could live inside would let the mutation through here."""
import numpy as np
import pytest

import hp_reference as H
import score_kernel_cases as K

pytestmark = pytest.mark.skipif(not H.AVAILABLE, reason="long double is not an extended type here")
CAUGHT = 10.0


def test_the_ard_cases_cover_what_they_claim():
    cs = K.ard_cases()
    assert len(set(cs)) == len(cs) == len(K.ARD_SIZES) * len(K.ARD_DS)
    assert {(c.n_pad, c.n) for c in cs} == set(K.ARD_SIZES) and {c.n for c in cs} >= {1, 2, 63, 64, 65, 128, 129, 200, 256, 384}
    for d in K.ARD_DS:
        assert {(c.kern, c.wsel) for c in cs if c.d == d} == {(k, w) for k in K.KERNEL_ID for w in K.WSEL}, d
    for fam in K.ARD_FAMILIES:
        assert {(c.kern, c.wsel) for c in cs if c.family == fam} == {(k, w) for k in K.KERNEL_ID for w in K.WSEL}, fam
        assert {c.members for c in cs if c.family == fam} == {1, 3}
    for n_pad in (128, 256, 384):
        assert {c.members for c in cs if c.n_pad == n_pad} == {1, 3}
        assert {K.ard_layout(c).tiles for c in cs if c.n_pad == n_pad} == {{128: 2, 256: 6, 384: 12}[n_pad]}
    assert all(c.n >= 2 for c in cs if c.family == "cluster")
    assert {K.ard_layout(c).dp for c in cs} == {64, 128}
    assert [K.tile_coords(t) for t in range(6)] == [(0, 0), (1, 0), (2, 0), (3, 0), (2, 1), (3, 1)]


@pytest.mark.parametrize("c", K.ard_cases(), ids=K.ard_id)
def test_ard_emulation_passes_and_every_mutation_is_caught(c):
    ops = K.ard_operands(c)
    out = K.ard_emulate(c, ops)
    refs = K.ard_reference(c, ops, out["Uc"])
    r = K.ard_judge(c, ops, out, refs)
    print("%s: emulation error / bound  Uc %.3g  partial %.3g  grad %.3g  noise %.3g;  error / S %.3g" % (K.ard_id(c), r["uc"], r["partial"], r["grad"], r["noise"], r["err_over_S"]))
    assert r["worst"] <= 1.0 and r["moved"] == 0 and r["uc_padding_zero"] and r["zero_columns"] and r["n1_zero"], r
    for mut in K.ARD_MUTATIONS:
        if not K.ard_mutation_applies(c, mut):
            continue
        rm = K.ard_judge(c, ops, K.ard_emulate(c, ops, mut), refs)
        print("    %-13s error / bound %.3g" % (mut, rm["partial"]))
        assert rm["partial"] >= CAUGHT, (mut, rm)


def test_a_group_member_is_emulated_like_the_member_alone():
    c = next(x for x in K.ard_cases() if x.members == 3 and x.n_pad == 256)
    ops = K.ard_operands(c)
    out = K.ard_emulate(c, ops)
    L = K.ard_layout(c)
    c1, ops1 = K.ard_member(c, ops, 1)
    out1 = K.ard_emulate(c1, ops1)
    assert K.same_bits(out1["partial"], out["partial"][L.sPartial:2 * L.sPartial]) and K.same_bits(out1["grad"], out["grad"][L.sGrad:2 * L.sGrad])


@pytest.mark.parametrize("c", K.band_cases(), ids=K.band_id)
def test_band_emulation_passes_and_a_shifted_block_is_caught(c):
    worst, moved = K.band_judge(c, K.band_emulate(c))
    bad, _ = K.band_judge(c, K.band_emulate(c, "block_shifted"))
    print("%s: emulation error / bound %.3g;  one K block shifted %.3g" % (K.band_id(c), worst, bad))
    assert worst <= 1.0 and moved == 0
    assert bad >= CAUGHT


@pytest.mark.parametrize("c", K.pred_cases(), ids=K.pred_id)
def test_predcov_emulation_passes_and_its_mutations_are_caught(c):
    part0, C0 = K.pred_emulate(c, finish=False)
    worst, moved = K.pred_judge_partial(c, part0, C0)
    partials = np.array(K.pred_partials_of(c, part0, C0))
    part, C = K.pred_emulate(c)
    fin, sym = K.pred_judge_finish(c, partials, C)
    print("%s: emulation error / bound  partial %.3g  finish %.3g" % (K.pred_id(c), worst, fin))
    assert worst <= 1.0 and moved == 0 and fin <= 1.0 and sym
    if c.S > 1:
        pm, Cm = K.pred_emulate(c, "slice_boundary", finish=False)
        bad, _ = K.pred_judge_partial(c, pm, Cm)
        print("    slice boundary off by one block: error / bound %.3g" % bad)
        assert bad >= CAUGHT
    _, Cm = K.pred_emulate(c, "mirror")
    bad, sym = K.pred_judge_finish(c, partials, Cm)
    print("    mirror not transposed: error / bound %.3g, symmetric %s" % (bad, sym))
    assert bad >= CAUGHT and not sym


def test_predcov_slicings_agree_within_their_bounds():
    for m_pad, fam in ((128, "cancel"), (256, "normal")):
        base = K.PredDesc(m_pad, 5, 1, fam, "kss", 1)
        C1 = K.pred_emulate(base)[1].astype(K.LD)
        for S in (2, 3, 5):
            cS = base._replace(S=S)
            CS = K.pred_emulate(cS)[1].astype(K.LD)
            assert np.all(np.abs(C1 - CS).reshape(m_pad, m_pad) <= K.pred_total_bound(base) + K.pred_total_bound(cS)), (m_pad, S)
