"""The exact per-ray problems of tests/exact_composite.py, proved on the CPU: every case tests/test_gpu_exact_composite.py runs satisfies its exactness
conditions (check_exact), and its fp64 reference is reproduced bit for bit by an f32 evaluation that takes every sum one addend at a time in two random
orders - and, for the transmittance problem, along the ray with the carry split at the 64-sample chunks.  Run with -s to see the figures per problem."""
import numpy as np
import pytest

import exact_composite as X


def _id(v):
    return str(v).replace(" ", "")


def _same(got, want):
    return got.dtype in (np.float32, np.uint8) and np.array_equal(got.astype(np.float64), np.asarray(want, dtype=np.float64))


@pytest.mark.parametrize("case", X.transmittance_cases(), ids=_id)
def test_transmittance_case_is_exact(case):
    form, pmod, bg, pad = case
    p = X.transmittance(form, pmod, bg, pad=pad)
    fig = X.check_exact(p)
    print("%s: %d samples in %d packs on %d rays; d sigma non-zero at %d (rgb / depth / alpha alone: %s); %d opaque samples behind a first one; tau scan <= %d "
          "quanta, sum |gw w| <= %.0f quanta of the 2^24 allowed" % (_id(case), fig.samples, fig.packs, fig.rays, fig.nonzero_d_sigma,
                                                                    list(fig.nonzero_single.values()), fig.opaque_behind, fig.tau_quanta, fig.gww_quanta))
    if pad:
        assert p.sigma_in.shape[0] == p.M + pad and np.isnan(p.sigma_in[p.M:]).all() and np.isnan(p.rgb_in[p.M:]).all() and int(p.pack_start[-1]) == p.M


@pytest.mark.parametrize("case", [c for c in X.transmittance_cases() if not c[3]], ids=_id)
def test_transmittance_reference_is_order_independent(case):
    """Forward and every backward in f32: two random orders, and the chunked scan with a carried total."""
    form, pmod, bg, _ = case
    p = X.transmittance(form, pmod, bg)
    want = X.reference(p)
    for kw in ({"order_seed": 1}, {"order_seed": 2}, {"chunked": True}):
        got = X.f32_transmittance(p, **kw)
        for name in ("weights", "alpha", "hit", "rgb", "depth"):
            assert _same(getattr(got, name), getattr(want, name)), (kw, name)
        for u in X.UPSTREAM:
            assert _same(got.d_sigma[u], want.d_sigma[u]) and _same(got.d_rgb[u], want.d_rgb[u]), (kw, u)


def test_transmittance_rays_without_pack_hold_the_background():
    for bg in (True, False):
        p = X.transmittance("permuted", 1, bg)
        r = X.reference(p)
        spare = ~p.has_pack
        assert spare.sum() == X.SPARE_RAYS
        assert (r.rgb[spare] == (1.0 if bg else 0.0)).all() and not r.alpha[spare].any() and not r.depth[spare].any() and not r.hit[spare].any()
        empty = p.has_pack & (p.len_of_ray == 0)
        assert empty.sum() >= 4 and (r.rgb[empty] == (1.0 if bg else 0.0)).all() and not r.alpha[empty].any()


@pytest.mark.parametrize("case", X.feature_cases() + [c + (X.PAD,) for c in X.FEATURE_PAD_CASES], ids=_id)
def test_feature_case_is_exact(case):
    p = X.features(*case[:3], pad=case[3] if len(case) > 3 else 0)
    fig = X.check_exact(p)
    print("%s: %d samples in %d packs on %d rays; per-ray sums <= %.0f eighths of the 2^24 allowed; d feats <= %d significant bits; %d rays with alpha = 0; "
          "%d non-zero outputs" % (_id(case), fig.samples, fig.packs, fig.rays, fig.sum_quanta, fig.d_feats_bits, fig.alpha_zero_rays, fig.nonzero_out))
    want = X.reference(p)
    assert np.array_equal(want.parts.sum(1)[np.argsort(p.ray_of_pack)], want.out[np.sort(p.ray_of_pack)])          # the quarters add up to the ray
    for seed in (1, 2):
        assert _same(X.f32_features(p, seed), want.out)


def test_feature_quarters_cover_the_edges():
    """The packs of 124..133 samples put 31, 32, 33 and 34 rows into a wave quarter: either side of the 32 rows the 64-wide bf16 kernel loads per iteration."""
    p = X.features("identity", 0, 64)
    rows = np.diff(X.quarters(p), axis=1)
    assert (rows.sum(1) == p.lens).all() and (rows >= 0).all()
    assert {31, 32, 33, 34} <= set(rows[:, 0].tolist())
    assert (rows[:, 3] == 0).any() and ((rows[:, 3] > 0) & (rows[:, 3] < rows[:, 0])).any()          # an empty and a short last quarter


@pytest.mark.parametrize("case", X.ray_sample_cases(), ids=_id)
def test_ray_sample_case_is_exact(case):
    p = X.ray_samples(*case)
    fig = X.check_exact(p)
    print("%s: %d samples in %d packs on %d rays; per-ray sums <= %.0f sixteenths of the 2^24 allowed" % (_id(case), fig.samples, fig.packs, fig.rays, fig.sum_quanta))
    want = X.reference(p)
    for seed in (1, 2):
        d_origins, d_dirs = X.f32_ray_samples(p, seed)
        assert _same(d_origins, want.d_origins) and _same(d_dirs, want.d_dirs)
    assert not want.d_origins[p.len_of_ray == 0].any() and not want.d_dirs[p.len_of_ray == 0].any()


def test_feature_weights_case_is_exact():
    p = X.feature_weights("boundary", 3)
    fig = X.check_exact(p)
    print("feature_weights: d sigma non-zero at %d of %d samples; |<g, f>| <= %.0f; d feats <= %d significant bits" % (fig.nonzero_d_sigma, fig.samples, fig.s_max, fig.d_feats_bits))


def test_pack_tables():
    """P % 4 in {0, 1, 3} for each of the three table forms; every listed length, empty packs first and last."""
    for form, pmod in X.TABLES:
        p = X.features(form, pmod, 7)
        assert p.P % 4 == pmod and int(p.pack_start[-1]) == p.M and (np.diff(p.pack_start) >= 0).all()
        assert len(set(p.ray_of_pack.tolist())) == p.P and p.ray_of_pack.max() < p.N
        if form == "identity":
            assert np.array_equal(p.ray_of_pack, np.arange(p.N)) and p.lens[0] == 0 and p.lens[-1] == 0
        if form == "boundary":
            assert p.boundary.sum() == p.P and np.array_equal(p.ray_of_sample[p.boundary], p.ray_of_pack)
